"""HET_HGTLayerHetero(use_norm=True): the per-node-type LayerNorm at the end of every forward path of the layer, in fp32 against the
fp64 oracle (oracle/layers.py::hgt_layer followed by the fp64 typed norm with the layer's parameters) and in bf16 against the staged
emulation of the rounding contract.  norm_weight ~ U(0.5, 1.5) and norm_bias ~ U(-1, 1) per type (ones and zeros would hide a wrong
type index); every gradient is taken for a random cotangent."""
import pytest
import torch

from tests._hgt_use_norm_ref import NORM_PARAMS, emulation, oracle
from tests.util import assert_close, mag_graph

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
MODES = [(False, True), (True, True), (False, False)]  # (hgt_fused_attn_score_flag, compact destinations)
SHAPES = [(8, 64, 64), (1, 64, 8), (2, 64, 10), (8, 64, 256), (4, 100, 64)]
NAMES = ["out", "grad_h"] + ["grad_" + n for n in NORM_PARAMS]


def _layer_graph():
    from het_amd.graph import HetGraph
    from het_amd.synth import make_random
    return HetGraph.from_integrated_coo(make_random(300, 4, 4000, seed=51, num_ntypes=3))  # (as tests/test_gpu_layers.py::test_hgt_layer)


def _new_layer(g, H, in_dim, out_dim, fused_attn=False, **kw):
    from het_amd.layers import HET_HGTLayerHetero
    torch.manual_seed(4)
    layer = HET_HGTLayerHetero(g.get_num_ntypes(), g.get_num_rels(), in_dim, out_dim, num_heads=H, dropout=0.0, use_norm=True,
                               hgt_fused_attn_score_flag=fused_attn, **kw)
    with torch.no_grad():
        layer.relation_pri.uniform_(0.5, 1.5)
        layer.skip.uniform_(-1, 1)
        layer.norm_weight.uniform_(0.5, 1.5)
        layer.norm_bias.uniform_(-1, 1)
    return layer


def _spy(monkeypatch):
    import het_amd.kernels as k
    calls = {}
    for name in ("rows_layer_norm", "rows_layer_norm_bf16", "rows_layer_norm_backward", "rows_layer_norm_backward_bf16"):
        real = getattr(k, name)

        def f(*a, _real=real, _name=name, **kw):
            calls.setdefault(_name, []).append(kw.get("save_stats"))
            return _real(*a, **kw)
        monkeypatch.setattr(k, name, f)
    return calls


def _run(g, layer, h, go):
    g.to_(DEV)
    layer = layer.to(DEV)
    hd = h.to(DEV).requires_grad_(True)
    out = layer(g, hd)
    out.backward(go.to(DEV))
    torch.cuda.synchronize()
    g.cpu_()
    return [out, hd.grad] + [getattr(layer, n).grad for n in NORM_PARAMS]


def _fp32_case(g, fused_attn, compact_dst, H, in_dim, out_dim, monkeypatch, **kw):
    from het_amd.backend import hgt_fused_layer
    monkeypatch.setattr(hgt_fused_layer, "COMPACT_DST_BELOW", 2.0 if compact_dst else 0.0)
    layer = _new_layer(g, H, in_dim, out_dim, fused_attn, **kw)
    N = g.get_num_nodes()
    h, go = torch.randn(N, in_dim) * 0.5, torch.randn(N, out_dim)
    ref = oracle(g, layer, h, go, H, fused_attn)
    calls = _spy(monkeypatch)
    got = _run(g, layer, h, go)
    kernel = out_dim % 4 == 0  # (10 columns: the torch composition)
    assert len(calls.get("rows_layer_norm", [])) == len(calls.get("rows_layer_norm_backward", [])) == int(kernel), calls
    for name, a, r in zip(NAMES, got, ref):
        assert_close(a, r, what=f"H={H} in={in_dim} out={out_dim} fused_attn={fused_attn} compact_dst={compact_dst} {name}")
    return layer, got


@pytest.mark.parametrize("fused_attn,compact_dst", MODES)
@pytest.mark.parametrize("H,in_dim,out_dim", SHAPES)
def test_fp32_layer(fused_attn, compact_dst, H, in_dim, out_dim, monkeypatch):
    """out, grad_h, the eight parameter gradients and norm_weight.grad / norm_bias.grad on the 300-node layer graph (its relations
    mix node types: the op-by-op composition)."""
    _fp32_case(_layer_graph(), fused_attn, compact_dst, H, in_dim, out_dim, monkeypatch)


@pytest.mark.parametrize("fused_attn,compact_dst", MODES)
@pytest.mark.parametrize("H,in_dim,out_dim", SHAPES)
def test_fp32_layer_fused_path(fused_attn, compact_dst, H, in_dim, out_dim, monkeypatch):
    """... and on a typed graph with canonical relations, where attention + aggregation run as one node, on the destinations with
    in-edges or on all nodes."""
    _fp32_case(mag_graph(1.5e-3), fused_attn, compact_dst, H, in_dim, out_dim, monkeypatch)


def test_fp32_layer_op_by_op(monkeypatch):
    from het_amd.backend import hgt_fused_layer
    monkeypatch.setattr(hgt_fused_layer, "FUSED", False)
    _fp32_case(mag_graph(1.5e-3), False, False, 2, 64, 64, monkeypatch)


def test_fp32_layer_multiply_among_weights_first(monkeypatch):
    from het_amd.backend import hgt_fused_layer
    monkeypatch.setattr(hgt_fused_layer, "FUSED", False)
    _fp32_case(mag_graph(1.5e-3), False, False, 1, 64, 64, monkeypatch, multiply_among_weights_first_flag=True)


def test_rows_without_in_edges_are_the_bias(monkeypatch):
    """A node without in-edges has y = 0: its output row is norm_bias[type] bitwise -- on the compact-destination path too, whose
    projection never computes those rows."""
    g = mag_graph(1.5e-3)
    layer, got = _fp32_case(g, False, True, 8, 64, 64, monkeypatch)
    N = g.get_num_nodes()
    indeg = torch.bincount(g.get_separate_coo_original()["col_indices"].cpu(), minlength=N)
    offs = g.get_original_node_type_offsets().cpu()
    types = torch.searchsorted(offs[1:].contiguous(), torch.arange(N), right=True)
    lone = indeg == 0
    assert int(lone.sum()) > 100 and len(set(types[lone].tolist())) > 1
    assert torch.equal(got[0].detach().cpu()[lone], layer.norm_bias.detach().cpu()[types[lone]])


def test_sampled_type_sorted_block_matches_full_graph():
    """Two use_norm layers on full-fan-out type-sorted blocks (runs of equal type, parameters through the per-run selection)
    reproduce the full-graph result on the seeds: values and the gradients of the input and of the norm's parameters."""
    from het_amd.graph import HetGraph
    from het_amd.sampling import NeighborSampler, run_blocks
    from het_amd.synth import make_mag_like
    coo = make_mag_like(scale=4e-4)
    for f in ("row", "col", "rel", "eids", "node_type_offsets"):
        setattr(coo, f, getattr(coo, f).cuda())
    g = HetGraph.from_integrated_coo(coo, full=True)
    N = coo.num_nodes
    layers = torch.nn.ModuleList([_new_layer(g, 4, 64, 64), _new_layer(g, 4, 64, 32)]).cuda()
    x = torch.randn(N, 64, device=DEV, requires_grad=True)
    full = x
    for layer in layers:
        full = layer(g, full)
    seeds = torch.randperm(N, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))[:40]
    blocks = NeighborSampler(g, [-1, -1], by_type=True).sample_blocks(seeds)
    assert blocks[-1].num_dst is not None and blocks[0].graph.graph_data["original"].get("node_segment_types") is not None
    order = blocks[-1].nodes[: blocks[-1].num_dst]
    go = torch.randn(order.numel(), 32, device=DEV)
    full[order].backward(go)
    want = [x.grad.clone()] + [p.grad.clone() for l in layers for p in (l.norm_weight, l.norm_bias)]
    x.grad = None
    layers.zero_grad()
    out = run_blocks(layers, blocks, x[blocks[0].nodes])
    out.backward(go)
    torch.testing.assert_close(out, full[order].detach(), rtol=2e-4, atol=2e-5)
    got = [x.grad] + [p.grad for l in layers for p in (l.norm_weight, l.norm_bias)]
    for a, b in zip(got, want):
        torch.testing.assert_close(a, b, rtol=2e-4, atol=1e-4)


def _rel(a, ref):
    return float((a.detach().double().cpu() - ref).norm() / ref.norm().clamp_min(1e-300))


def _bf16_case(g, fused_attn, compact_dst, H, in_dim, out_dim, monkeypatch, native):
    """d_hip <= max(2 d_ref, 1e-5) for the output and every gradient (the criterion of tests/test_gpu_hgt_bf16.py::_layer_case): d_ref
    the distance of the staged emulation to the fp64 oracle, d_hip that of the layer, both on the same bf16-rounded h / cotangent."""
    from het_amd.backend import hgt_fused_layer
    monkeypatch.setattr(hgt_fused_layer, "COMPACT_DST_BELOW", 2.0 if compact_dst else 0.0)
    layer = _new_layer(g, H, in_dim, out_dim, fused_attn)
    N = g.get_num_nodes()
    hb, gob = (torch.randn(N, in_dim) * 0.5).to(BF16), torch.randn(N, out_dim).to(BF16)
    ref, emu = oracle(g, layer, hb, gob, H, fused_attn), emulation(g, layer, hb, gob, H, fused_attn)
    calls = _spy(monkeypatch)
    got = _run(g, layer, hb, gob)
    assert got[0].dtype == BF16 and got[1].dtype == BF16 and got[0].shape == (N, out_dim)
    assert all(bool(torch.isfinite(t.float()).all()) for t in got)
    if native:  # the bf16 kernel ran once, forward and backward; its fp32 twin did not
        assert len(calls.get("rows_layer_norm_bf16", [])) == 1 and len(calls.get("rows_layer_norm_backward_bf16", [])) == 1, calls
        assert "rows_layer_norm" not in calls and "rows_layer_norm_backward" not in calls, calls
    else:
        assert "rows_layer_norm_bf16" not in calls, calls
    bad = []
    for name, a, r, e in zip(NAMES, got, ref, emu):
        if name not in ("out", "grad_h"):
            assert a.dtype == torch.float32, name
        d_ref, d_hip = _rel(e, r), _rel(a, r)
        print(f"use_norm H={H} in={in_dim} out={out_dim} fused_attn={fused_attn} compact_dst={compact_dst} {name}: d_ref {d_ref:.3e} d_hip {d_hip:.3e}")
        if not d_hip <= max(2 * d_ref, 1e-5):
            bad.append((name, d_ref, d_hip))
    assert not bad, bad


@pytest.mark.parametrize("fused_attn,compact_dst", MODES)
@pytest.mark.parametrize("H,in_dim,out_dim", [(8, 64, 64), (1, 32, 32)])
def test_bf16_layer_native(fused_attn, compact_dst, H, in_dim, out_dim, monkeypatch):
    _bf16_case(mag_graph(1.5e-3), fused_attn, compact_dst, H, in_dim, out_dim, monkeypatch, native=True)


def test_bf16_layer_upcast(monkeypatch):
    """A shape without bf16 kernels (heads of 5, 10 output columns): fp32 on an upcast copy, the norm inside it, one rounding."""
    _bf16_case(mag_graph(1.5e-3), False, True, 2, 64, 10, monkeypatch, native=False)


@pytest.mark.parametrize("dtype", [torch.float32, BF16])
def test_evaluation_saves_nothing_and_changes_no_bits(dtype, monkeypatch):
    g = mag_graph(1.5e-3)
    layer = _new_layer(g, 8, 64, 64).to(DEV)
    h = (torch.randn(g.get_num_nodes(), 64) * 0.5).to(dtype).to(DEV)
    calls = _spy(monkeypatch)
    g.to_(DEV)
    train = layer(g, h)
    with torch.no_grad():
        ev = layer(g, h)
    g.cpu_()
    assert torch.equal(train, ev)
    assert calls["rows_layer_norm_bf16" if dtype == BF16 else "rows_layer_norm"] == [True, False]  # (save_stats per call)


def test_train_driver_use_norm(capsys):
    """python -m het_amd.train --model hgt --use_norm: one epoch on the small synthetic mag graph of the driver's own test; the flag is in the logged args,
    and a run without it logs the line it logged before."""
    from het_amd import train
    common = ["--model", "hgt", "-d", "mag", "--scale", "0.002", "--full_graph_training", "--n_infeat", "64", "--num_classes", "64",
              "--num_heads", "4", "--num_layers", "2", "--n_epochs", "1", "--dropout", "0.0", "--no_warm_up"]
    res = train.main(common + ["--use_norm"])
    assert res["args"]["use_norm"] is True and res["final_loss"] == res["final_loss"] and res["mean_backward_ms"] > 0
    assert '"use_norm": true' in capsys.readouterr().out
    plain = train.main(common)
    assert "use_norm" not in plain["args"]
