"""No result may depend on what an uninitialised buffer held.  Every case below is an existing case function of the suite -- its
fp64 oracle, its tolerance, its assertions, unchanged -- run inside tests/_poison.py::poisoned, which fills every floating-point
tensor that het_amd's Python takes from torch.empty / empty_like / empty_strided / new_empty with NaN or with 1e30 before the
library sees it: sm, ret, feat_c, el_c, er_c, the run sums, the gradient buffers, every _workspace scratch buffer.  A kernel that
reads a slot it never wrote, adds into a buffer it took for zero, or multiplies an unwritten row by a zero weight passes on recycled
memory and fails here.  NaN alone would not do: fmaxf(NaN, x) = x, a running-maximum slot swallows it (tests/test_poison_harness.py).

Every case asserts that something was poisoned at all, and the cases that reach a kernels._workspace buffer (hub partials, the
compact backwards, rgcn_layer_backward) that one of those was.  Out of reach, by design: integer tensors (a poisoned index is an
out-of-range address), the library's own allocator (groupings and their construction scratch: index arrays), tensors a caller hands
in (the op tests pre-fill those) and at::empty inside the compiled registration.  With HET_TORCH_HRT_LIB set, the reference-named
torch_hrt ops are served by that compiled object: the cases that go through them (the op-by-op HGT layer and the HGT CSR composition)
then poison only what the Python around them allocates and do not assert a record.

The bitwise leg runs the default fp32 training step of the three layers unpoisoned, under NaN and under 1e30 on a graph without a
segment or destination above 256 positions (no float atomics) and requires torch.equal on the output and every gradient."""
import pytest
import torch

import tests.test_gpu_bf16_ladders as BL
import tests.test_gpu_hgt_bf16 as HB
import tests.test_gpu_hgt_csr as HC
import tests.test_gpu_layers as L
import tests.test_gpu_ops as T
import tests.test_gpu_rgat_attention as AT
import tests.test_gpu_rgat_backward_routes as RT
import tests.test_gpu_rgat_bf16 as FB
import tests.test_gpu_rgat_bf16_train as TB
import tests.test_gpu_rgat_forward_only as FO
import tests.test_gpu_rgcn_bf16 as CB
import tests.test_sampling as SM
from oracle import layers as OL
from tests._poison import POISON_IDS, POISONS, poisoned
from tests.test_gpu_ops import K  # noqa: F401  (fixture)
from tests.test_gpu_thresholds import ladder  # noqa: F401  (fixture: ladder_graph(R=5, seed=0), checked with assert_ladder)
from tests.util import assert_close, assert_ladder, ladder_counts, ladder_graph, random_graph, rgat_min_abs_preactivation

pytestmark = pytest.mark.gpu
DEV = "cuda"
poison = pytest.mark.parametrize("value", POISONS, ids=POISON_IDS)
_checked = []


def _under(value, fn, *args, workspace=False, record=True, **kwargs):
    """fn(*args, **kwargs) with het_amd's uninitialised float tensors poisoned; the patch is gone again before anything is judged.
    workspace: a kernels._workspace buffer must be among them."""
    with poisoned(value) as rec:
        out = fn(*args, **kwargs)
        torch.cuda.synchronize()
    if record:
        assert rec, "nothing was poisoned: the case allocates nothing through het_amd's Python"
        assert all(m.startswith("het_amd") for m in rec.modules()), rec.modules()
    if workspace:
        assert rec.from_module("het_amd.kernels", "_workspace"), sorted({(e.module, e.function) for e in rec})
    return out


def _layer_ladder(R=5):
    """The ladder graph as the layers take it (canonical eids): hubs of 257 / 513 in-edges, nodes without edges, an empty relation,
    destinations split over relations.  A new object per case (the case functions move it to the GPU and back)."""
    g = ladder_graph(R=R, seed=0, shuffle=False)
    if R not in _checked:
        assert_ladder(g)
        _checked.append(R)
    return g


def _small():
    return random_graph(seed=41, n=400, r=4, e=6000, shuffle=False)


def _python_registration():
    import het_amd.kernels as k
    return k.COMPILED_LIB is None


# ---------------------------------------------------------------- RGAT layer, fp32 training
@poison
@pytest.mark.parametrize("compact,direct,mulfirst", [(False, False, False), (False, False, True), (True, False, False),
                                                     (True, True, False), (True, True, True), (True, False, True)])
def test_rgat_layer_variants_on_the_ladder(compact, direct, mulfirst, value):
    _under(value, L._run_rgat, _layer_ladder(), H=4, K=64, X=64, compact=compact, direct=direct, mulfirst=mulfirst, workspace=True)


@poison
@pytest.mark.parametrize("self_loop,bias", [(True, False), (False, True), (False, False)])
def test_rgat_layer_without_self_loop_or_bias(self_loop, bias, value):
    """No self-loop: there are no self-loop rows for the aggregation to add into (h is None in _loop_and_bias_rows) -- the rows of
    destinations without in-edges are then written by nobody but the layer's own fill."""
    _under(value, L._run_rgat, _layer_ladder(), H=4, K=64, X=64, compact=False, direct=False, mulfirst=True, self_loop=self_loop, bias=bias,
           workspace=True)


@poison
@pytest.mark.parametrize("H,K,X,pad", [(4, 48, 64, True), (4, 64, 16, True), (4, 64, 16, False), (2, 48, 24, True)])
def test_rgat_layer_widths_outside_the_fused_shapes(H, K, X, pad, value, monkeypatch):
    """K = 48 is outside the fused self-loop product and the matrix-core projection (zero-padded columns), X = 16 gives heads of 4
    floats: padded to the row kernels' widths, or (pad off) the any-shape projection and the row-dot for el_c."""
    import het_amd.layers as HL
    monkeypatch.setattr(HL, "PAD_HEADS", pad)
    _under(value, L._run_rgat, _layer_ladder(), H=H, K=K, X=X, compact=True, direct=True, mulfirst=True)


@poison
@pytest.mark.parametrize("mulfirst", [False, True])
def test_rgat_layer_per_edge_dataflow(mulfirst, value, monkeypatch):
    from het_amd.backend import rgat_fused_layer as FL
    monkeypatch.setattr(FL, "PER_EDGE", True)
    _under(value, L._run_rgat, _layer_ladder(), H=4, K=64, X=64, compact=False, direct=False, mulfirst=mulfirst)


@poison
@pytest.mark.parametrize("overlap", [True, False])
@pytest.mark.parametrize("self_loop,bias", RT.LOOP_BIAS)
@pytest.mark.parametrize("graph", ["whole", "block"])
def test_rgat_node_major_route(graph, self_loop, bias, overlap, value, monkeypatch):
    _under(value, RT._run, monkeypatch, "node-major", graph, 4, 64, 64, True, self_loop, bias, overlap, workspace=True)


@poison
@pytest.mark.parametrize("self_loop,bias", RT.LOOP_BIAS)
@pytest.mark.parametrize("mulfirst", [True, False])
def test_rgat_generic_route(mulfirst, self_loop, bias, value, monkeypatch):
    _under(value, RT._run, monkeypatch, "generic", "whole", 4, 64, 128, mulfirst, self_loop, bias, True, workspace=True)


@poison
def test_rgat_edges_ending_at_or_above_num_dst(value, monkeypatch):
    """num_dst < N with edges that end at or above it: th.zeros_like(x) instead of th.empty_like(x) is what keeps the rows of grad_x
    that no relation writes."""
    _under(value, RT._run, monkeypatch, "generic", "whole_num_dst", 4, 64, 64, True, True, True, True, workspace=True)


@poison
@pytest.mark.parametrize("compact", [False, True])
def test_rgat_on_sampled_blocks(compact, value):
    """Two layers over NeighborSampler(g, [4, 6], seed=3) blocks: num_dst < N in both."""
    _under(value, SM.test_rgat_on_sampled_blocks_matches_the_oracle_on_the_blocks, compact, False)


def _halo_case(world, chunks, monkeypatch):
    """tests/test_gpu_dist.py::test_eight_way_partition_feat128_on_one_gpu at a size for every run of the suite: the graph split by
    destination range over ``world`` logical ranks (dist.LocalRanks), the halo exchange in ``chunks`` pieces, every rank through
    forward_with_halo; outputs, input gradients and the summed parameter gradients against the fp64 oracle on the whole graph."""
    import het_amd.dist as D
    from het_amd.graph import HetGraph
    from het_amd.layers import HET_RGATLayer
    from het_amd.synth import make_random
    monkeypatch.setattr(D, "CHUNKS", chunks)
    feat, H = 64, 4
    coo = make_random(600, 4, 9000, seed=41)
    torch.manual_seed(0)
    layer = HET_RGATLayer(feat, feat, coo.num_rels, H, self_loop=True, dropout=0.0)
    with torch.no_grad():
        layer.h_bias.uniform_(-0.1, 0.1)
    gen = torch.Generator().manual_seed(2)
    x, go = torch.randn(coo.num_nodes, feat, generator=gen) * 0.5, torch.randn(coo.num_nodes, feat, generator=gen)
    s = HetGraph.from_integrated_coo(coo).get_separate_coo_original()
    for _ in range(64):  # (no pre-activation on the leaky-ReLU kink: tests/util.py)
        if rgat_min_abs_preactivation(x, layer.conv_weights, layer.attn_l, layer.attn_r, s) >= 2e-6:
            break
        x = x + 1e-3 * torch.randn(coo.num_nodes, feat, generator=gen)
    names = ["conv_weights", "attn_l", "attn_r", "loop_weight", "h_bias"]
    p64 = {n: t.detach().double().requires_grad_(True) for n, t in layer.named_parameters()}
    x64 = x.double().requires_grad_(True)
    ref = OL.rgat_layer(x64, p64["conv_weights"], p64["attn_l"], p64["attn_r"], s["rel_ptrs"], s["row_indices"], s["col_indices"],
                        coo.num_nodes, 0.2, p64["loop_weight"], p64["h_bias"])
    grads_ref = torch.autograd.grad(ref, [x64] + [p64[n] for n in names], go.double())
    layer = layer.to(DEV)
    dcoo = make_random(600, 4, 9000, seed=41)
    for f in ("row", "col", "rel", "eids", "node_type_offsets"):
        setattr(dcoo, f, getattr(dcoo, f).to(DEV))
    lr = D.LocalRanks(dcoo, world, layer)
    assert all(p.chunks == chunks for p in lr.plans) and sum(p.n_halo for p in lr.plans) > 0
    mine = [lr.owned_nodes(r).cpu() for r in range(world)]
    x_own = [x[m].to(DEV).requires_grad_(True) for m in mine]
    outs = lr.forward(x_own)
    assert all(lr.took_halo_path), lr.took_halo_path
    lr.backward(outs, [go[m].to(DEV) for m in mine], x_own)
    torch.cuda.synchronize()
    for r in range(world):
        assert_close(outs[r], ref.detach()[mine[r]], what=f"rank {r} out")
        assert_close(x_own[r].grad, grads_ref[0][mine[r]], what=f"rank {r} grad_x")
    for n, gr in zip(names, grads_ref[1:]):
        assert_close(dict(layer.named_parameters())[n].grad, gr, what=f"grad_{n} (sum over the ranks)")


@poison
@pytest.mark.parametrize("chunks", [1, 4])
def test_rgat_halo_route(chunks, value, monkeypatch):
    _under(value, _halo_case, 3, chunks, monkeypatch, workspace=True)


# ---------------------------------------------------------------- RGAT layer, other modes
@poison
def test_rgat_forward_only_fp32(value, monkeypatch):
    """Under torch.no_grad(), bit-identical to the training forward and within the oracle's tolerance, on the ladder graph."""
    _under(value, FO.test_bit_identity_ladder_graph_with_hubs, 5, 4, 16, monkeypatch, workspace=True)


@poison
@pytest.mark.parametrize("self_loop,bias", [(True, False), (False, True), (False, False)])
def test_rgat_forward_only_without_self_loop_or_bias(self_loop, bias, value, monkeypatch):
    _under(value, FO.test_bit_identity_without_self_loop_or_bias, self_loop, bias, monkeypatch)
    _under(value, FO.test_empty_relation_and_nodes_without_in_edges, monkeypatch)


@poison
@pytest.mark.parametrize("name", ["hub_el_from_row", "hub_el_gathered", "loop0_bias0", "block_num_dst_no_loop"])
def test_rgat_forward_only_bf16(name, value, monkeypatch):
    _under(value, FB.test_values_against_the_staged_reference, name, monkeypatch)


@poison
@pytest.mark.parametrize("kind,R,H,D", [("ladder", 5, 4, 16), ("ladder", 5, 2, 32)])
def test_rgat_get_attention(kind, R, H, D, value, monkeypatch):
    """get_attention=True under torch.no_grad(): fp32 and bf16 rows (the lse of destinations without in-edges is -inf by design)."""
    _under(value, AT.test_values_fp32, kind, R, H, D, monkeypatch, workspace=True)
    monkeypatch.undo()
    _under(value, AT.test_values_bf16, kind, R, H, D, monkeypatch, workspace=True)


@poison
@pytest.mark.parametrize("name", ["ladder_el_from_row", "ladder_el_gathered", "block_num_dst"])
def test_rgat_bf16_training(name, value, monkeypatch):
    _under(value, TB.test_values_against_the_staged_emulation, name, monkeypatch, workspace=True)


# ---------------------------------------------------------------- RGCN layer
@poison
@pytest.mark.parametrize("compact", [False, True])
def test_rgcn_layer_on_the_ladder(compact, value, monkeypatch):
    """compact off: the two-call layer (rgcn_layer_forward / rgcn_layer_backward: ssum, grad_x, grad_w, grad_bias and the backward's
    workspace are all uninitialised); compact on: the a7 / a8 pair."""
    import het_amd.kernels as k
    calls = []
    real = k.rgcn_layer_backward
    monkeypatch.setattr(k, "rgcn_layer_backward", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    _under(value, L._run_rgcn, _layer_ladder(), compact, compact, 64, 64, 5, workspace=not compact)
    assert len(calls) == (0 if compact else 1)


@poison
@pytest.mark.parametrize("Kd,D,R", [(64, 16, 5), (64, 64, 9)])
def test_rgcn_layer_padded_width_and_nine_relations(Kd, D, R, value):
    """D = 16: the output width zero-padded to 32; R = 9: outside rgcn_layer_ok, the pair of reference-named ops."""
    import het_amd.kernels as k
    assert k.rgcn_layer_ok(R, Kd, 32 if D == 16 else D) == (R < 8)
    _under(value, L._run_rgcn, _layer_ladder(R), False, False, Kd, D, R)


@poison
def test_rgcn_bf16_step(value):
    g = ladder_graph(R=3, seed=6)
    _under(value, CB._bf16_step, g, 64, 64, 3, workspace=True)


@poison
def test_rgcn_on_a_sampled_block(value):
    """The first block of NeighborSampler(g, [4, 6], seed=3): num_dst < N, the rows of the source-only nodes are not returned."""
    from het_amd.sampling import NeighborSampler
    g = _small()
    b = NeighborSampler(g, [4, 6], seed=3).sample_blocks(torch.tensor([7, 300, 42, 9, 111, 250, 18, 77]))[0]
    assert b.num_dst < b.graph.get_num_nodes()
    _under(value, L._run_rgcn, b.graph, False, False, 64, 64, 4, num_dst=b.num_dst)


# ---------------------------------------------------------------- HGT layer
@poison
@pytest.mark.parametrize("fused_attn,compact_dst", [(False, True), (True, True), (False, False)])
def test_hgt_layer_fused(fused_attn, compact_dst, value, monkeypatch):
    _under(value, L._run_hgt_fused, fused_attn, compact_dst, 8, 64, 64, monkeypatch, workspace=True)


@poison
def test_hgt_layer_fused_on_the_ladder(value, monkeypatch):
    """Hub destinations: the aggregation parks their partial sums in its workspace."""
    _under(value, L._run_hgt_fused, False, True, 4, 64, 64, monkeypatch, g=_layer_ladder(), workspace=True)


@poison
@pytest.mark.parametrize("native,H,in_dim,out_dim", [(True, 8, 64, 64), (False, 2, 64, 10)])
def test_hgt_bf16_layer(native, H, in_dim, out_dim, value, monkeypatch):
    _under(value, HB._layer_case, HB._hub_graph(), False, True, H, in_dim, out_dim, monkeypatch, native=native, workspace=True)


@poison
@pytest.mark.parametrize("fused_attn,compact,direct", [(False, False, False), (True, False, False), (False, True, True)])
def test_hgt_layer_op_by_op(fused_attn, compact, direct, value, monkeypatch):
    """The single-node path off: the composition of the reference-named ops (het_amd/backend/hgt_layers_and_funcs.py)."""
    from het_amd.backend import hgt_fused_layer
    monkeypatch.setattr(hgt_fused_layer, "FUSED", False)
    _under(value, L.test_hgt_layer, fused_attn, compact, direct, 8, 64, 64, record=_python_registration())


@poison
@pytest.mark.parametrize("graph", ["random", "hub"])
def test_hgt_csr_composition(graph, value):
    _under(value, HC.test_hgt_csr_composition_matches_fused_coo, True, graph, 8, 8, record=_python_registration())


# ---------------------------------------------------------------- ops that allocate internally, on the ladder graph
@poison
@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("H,D", [(4, 16), (1, 64), (2, 32)])
def test_rgat_run_sums_op(K, ladder, H, D, fold, value):
    _under(value, T.rgat_run_sums_case, K, ladder, H, D, fold=fold, bias=fold, workspace=True)


@poison
@pytest.mark.parametrize("H,D", [(4, 16), (8, 8), (2, 4)])
def test_rgat_compact_op(K, ladder, H, D, value):
    _under(value, T.rgat_compact_case, K, ladder, H, D, fold=True, bias=True, workspace=True)


@poison
@pytest.mark.parametrize("H,D", [(8, 8), (1, 64)])
def test_hgt_compact_op(K, ladder, H, D, value):
    _under(value, T.hgt_compact_case, K, ladder, H, D, workspace=True)


@poison
@pytest.mark.parametrize("H,D", [(4, 16), (2, 32)])
def test_rgat_bf16_gather_passes_op(ladder, H, D, value):
    _under(value, BL.rgat_gather_passes_case, ladder, H, D, fold=True, bias=True, workspace=True)


@poison
@pytest.mark.parametrize("H,D", [(8, 8), (1, 64)])
def test_hgt_bf16_compact_op(ladder, H, D, value):
    _under(value, HB._op_case, ladder, H, D, workspace=True)


@poison
@pytest.mark.parametrize("H", [4, 1])
def test_rgat_attention_compact_op(H, value):
    """With and without lse_out (without it the lse lives in the workspace), on the shuffled ladder graph."""
    _under(value, AT.test_lse_out_of_the_library_call, H, workspace=True)


@poison
@pytest.mark.parametrize("fused_attn", [False, True])
def test_hgt_fold_source_weights_op(fused_attn, value, monkeypatch):
    _under(value, L.test_hgt_fold_kernel_matches_the_torch_composition, 3, 5, 8, 8, 64, fused_attn, monkeypatch)


@poison
@pytest.mark.parametrize("Kd,X,bias", [(64, 64, True), (32, 128, False), (128, 32, True)])
def test_rows_linear_bias_allocates_its_output(Kd, X, bias, value):
    """out=None: the op allocates [n, X] itself and must write every row of [offsets[0], offsets[1]) -- 1000 rows: not a multiple of
    the 32- and 64-row tiles."""
    import het_amd.kernels as k
    assert k.rows_linear_bias_ok(Kd, X)
    gen = torch.Generator().manual_seed(Kd + X)
    n = 1000
    x, w, b = torch.randn(n, Kd, generator=gen), torch.randn(Kd, X, generator=gen) * 0.2, torch.randn(X, generator=gen)
    offs = torch.tensor([0, n], dtype=torch.int64, device=DEV)
    out = _under(value, k.rows_linear_bias, offs, x.to(DEV), w.to(DEV), b.to(DEV) if bias else None)
    assert_close(out, x.double() @ w.double() + (b.double() if bias else 0.0), what="x . w + bias")


# ---------------------------------------------------------------- the bitwise leg
def _bitwise_graph():
    """random_graph(seed=41, n=400, r=4, e=6000): no (relation, source) or (relation, destination) segment, no destination and no
    source above 256 positions -- nothing is split over work items, no float atomics run, and a step's bits are reproducible (the
    argument of tests/test_gpu_ops.py::test_rgat_backward_packs_do_not_depend_on_the_groupings_first_user)."""
    g = _small()
    c = ladder_counts(g)
    s = g.get_separate_coo_original()
    out_deg = torch.bincount(s["row_indices"], minlength=g.get_num_nodes())
    assert max(int(c["in_rel"].max()), int(c["in"].max()), int(c["out_rel"].max()), int(out_deg.max())) <= 256
    return g


def _rgat_step(g):
    from het_amd.layers import HET_RGATLayer
    torch.manual_seed(3)
    layer = HET_RGATLayer(64, 64, g.get_num_rels(), 4, self_loop=True, dropout=0.0).to(DEV)
    x = (torch.randn(g.get_num_nodes(), 64) * 0.5).to(DEV).requires_grad_(True)
    out = layer(g, x)
    out.backward(torch.randn(g.get_num_nodes(), 64).to(DEV))
    return layer, x, out.detach()


def _rgcn_step(g):
    from het_amd.layers import HET_EglRelGraphConv_EdgeParallel
    torch.manual_seed(3)
    layer = HET_EglRelGraphConv_EdgeParallel(64, 64, g.get_num_rels(), bias=True).to(DEV)
    x = torch.randn(g.get_num_nodes(), 64).to(DEV).requires_grad_(True)
    norm = torch.rand(g.get_num_edges(), 1).to(DEV)
    out = layer(g, x, norm)
    out.backward(torch.randn(g.get_num_nodes(), 64).to(DEV))
    return layer, x, out.detach()


def _hgt_step(g):
    from het_amd.layers import HET_HGTLayerHetero
    torch.manual_seed(3)
    layer = HET_HGTLayerHetero(g.get_num_ntypes(), g.get_num_rels(), 64, 64, num_heads=8, dropout=0.0)
    with torch.no_grad():
        layer.relation_pri.uniform_(0.5, 1.5)
        layer.skip.uniform_(-1, 1)
    layer = layer.to(DEV)
    x = (torch.randn(g.get_num_nodes(), 64) * 0.5).to(DEV).requires_grad_(True)
    out = layer(g, x)
    out.backward(torch.randn(g.get_num_nodes(), 64).to(DEV))
    return layer, x, out.detach()


# Left out of the leg, measured before it was written (40 unpoisoned steps on this graph: 4 bit patterns for this tensor, one for every
# other tensor of the three steps): the RGAT attention-vector gradient is finished by csrc/gat_compact.hip::HET_rgat_attn_grad_finish,
# whose lane groups add their partial rows with float atomics whatever the segment lengths are.  Its values are held against the fp64
# oracle, poisoned, by every RGAT case above.
NOT_BIT_REPRODUCIBLE = {"rgat": {"grad_attn_l"}, "rgcn": set(), "hgt": set()}


@pytest.mark.parametrize("model", ["rgat", "rgcn", "hgt"])
def test_training_step_bits_do_not_depend_on_the_poison(model):
    """The default fp32 training step, forward + backward: the same bits unpoisoned (twice: the step is reproducible to begin with),
    under NaN and under 1e30 -- the output, grad_x and every parameter gradient."""
    step = {"rgat": _rgat_step, "rgcn": _rgcn_step, "hgt": _hgt_step}[model]
    g = _bitwise_graph()
    g.to_(DEV)

    def run(value=None):
        layer, x, out = step(g) if value is None else _under(value, step, g, workspace=True)
        torch.cuda.synchronize()
        got = {"out": out.clone(), "grad_x": x.grad.clone()}
        got.update({"grad_" + n: p.grad.clone() for n, p in layer.named_parameters() if p.grad is not None})
        return got

    plain, again = run(), run()
    assert set(plain) == set(again) and len(plain) > 3
    for n in set(plain) - NOT_BIT_REPRODUCIBLE[model]:
        assert torch.equal(plain[n], again[n]), f"{model} {n}: two unpoisoned steps differ -- the route is not bit-reproducible"
    for value, vid in zip(POISONS, POISON_IDS):
        got = run(value)
        assert set(got) == set(plain)
        for n in set(plain) - NOT_BIT_REPRODUCIBLE[model]:
            assert bool(torch.isfinite(got[n]).all()), f"{model} {n} under {vid}"
            assert torch.equal(got[n], plain[n]), f"{model} {n}: the bits depend on uninitialised memory ({vid})"
    g.cpu_()
