"""The RGAT layer's forward-only path (evaluation: torch.no_grad(), or nothing that requires a gradient): which calls take it,
that its output is BIT-IDENTICAL to the training forward's (only stores and what feeds them were removed), that it matches the
fp64 oracle, and that the tensors it no longer allocates are gone from the peak."""
import json

import pytest
import torch

from oracle import layers as OL
from tests.util import assert_close, ladder_graph, mag_graph, random_graph

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _count_calls(monkeypatch):
    import het_amd.kernels as k
    calls = {"forward_only": 0, "training": 0}
    fo, tr = k.rgat_aggregate_compact_forward, k.rgat_aggregate_compact

    def f(*a, **kw):
        calls["forward_only"] += 1
        return fo(*a, **kw)

    def t(*a, **kw):
        calls["training"] += 1
        return tr(*a, **kw)

    monkeypatch.setattr(k, "rgat_aggregate_compact_forward", f)
    monkeypatch.setattr(k, "rgat_aggregate_compact", t)
    return calls


def _layer(g, H, K, X, mulfirst=False, self_loop=True, bias=True, seed=0, **kw):
    from het_amd.layers import HET_RGATLayer
    torch.manual_seed(seed)
    layer = HET_RGATLayer(K, X, g.get_num_rels(), H, bias=bias, self_loop=self_loop, multiply_among_weights_first_flag=mulfirst,
                          dropout=0.0, **kw)
    if bias:
        with torch.no_grad():
            layer.h_bias.uniform_(-0.1, 0.1)
    x = torch.randn(g.get_num_nodes(), K) * 0.5
    return layer.to(DEV), x.to(DEV)


def _both(g, layer, x, calls, num_dst=None):
    """(forward-only output under no_grad, training forward's output with gradients on), each checked for the path it took."""
    before = dict(calls)
    with torch.no_grad():
        out_f = layer(g, x, num_dst)
    assert (calls["forward_only"] - before["forward_only"], calls["training"] - before["training"]) == (1, 0), calls
    assert not out_f.requires_grad and out_f.grad_fn is None
    out_t = layer(g, x, num_dst)
    assert (calls["forward_only"] - before["forward_only"], calls["training"] - before["training"]) == (1, 1), calls
    assert out_t.requires_grad
    return out_f, out_t.detach()


def _oracle(g_cpu_lists, layer, x, N, nd=None):
    s = g_cpu_lists
    p = {n: t.detach().cpu().double() for n, t in layer.named_parameters()}
    ref = OL.rgat_layer(x.detach().cpu().double(), p["conv_weights"], p["attn_l"], p["attn_r"], s["rel_ptrs"].cpu(), s["row_indices"].cpu(),
                        s["col_indices"].cpu(), N, 0.2, p.get("loop_weight"), p.get("h_bias"))
    return ref if nd is None else ref[:nd]


def test_path_selection(monkeypatch):
    from het_amd.backend import rgat_fused_layer as FL
    calls = _count_calls(monkeypatch)
    g = random_graph(seed=700, n=300, r=4, e=5000, shuffle=False)
    layer, x = _layer(g, 4, 64, 64)
    g.to_(DEV)
    with torch.no_grad():  # autograd off
        out = layer(g, x)
    assert calls == {"forward_only": 1, "training": 0}
    assert out.requires_grad is False and out.grad_fn is None
    for p in layer.parameters():  # autograd on, nothing asks for a gradient
        p.requires_grad_(False)
    out2 = layer(g, x)
    assert calls == {"forward_only": 2, "training": 0}
    assert out2.requires_grad is False and out2.grad_fn is None and torch.equal(out, out2)
    out3 = layer(g, x.clone().requires_grad_(True))  # ... but the input does
    assert calls == {"forward_only": 2, "training": 1} and out3.grad_fn is not None
    for p in layer.parameters():  # parameters that train: the autograd node
        p.requires_grad_(True)
    out4 = layer(g, x)
    assert calls == {"forward_only": 2, "training": 2} and out4.grad_fn is not None
    # HET_RGAT_FORWARD_ONLY=0 (read when the module is imported, like HET_RGAT_PER_EDGE): today's behaviour
    monkeypatch.setattr(FL, "FORWARD_ONLY", False)
    with torch.no_grad():
        out5 = layer(g, x)
    assert calls == {"forward_only": 2, "training": 3}
    assert torch.equal(out5, out)
    g.cpu_()


@pytest.mark.parametrize("H,D,R", [(4, 16, 4), (2, 16, 8), (2, 32, 4), (1, 32, 3), (1, 64, 4), (8, 16, 5), (4, 16, 9)])
@pytest.mark.parametrize("mulfirst", [False, True])
def test_bit_identity_shapes(H, D, R, mulfirst, monkeypatch):
    """Every row width of the run-sum form; el from the gathered row (D = 16, R <= 8) and gathered (D = 32 / 64, or 9 relations);
    er from the folded weight and from the projection (HET_RGAT_LITERAL_ER keeps the latter)."""
    from het_amd.backend import rgat_fused_layer as FL
    if not mulfirst:
        monkeypatch.setattr(FL, "LITERAL_ER", True)
    calls = _count_calls(monkeypatch)
    g = random_graph(seed=710 + R, n=400, r=R, e=9000, shuffle=False, empty_rel=R > 2)
    layer, x = _layer(g, H, 64, H * D, mulfirst=mulfirst, seed=H + D)
    g.to_(DEV)
    out_f, out_t = _both(g, layer, x, calls)
    g.cpu_()
    assert torch.equal(out_f, out_t), float((out_f - out_t).abs().max())


@pytest.mark.parametrize("self_loop,bias", [(True, False), (False, True), (False, False)])
def test_bit_identity_without_self_loop_or_bias(self_loop, bias, monkeypatch):
    calls = _count_calls(monkeypatch)
    g = random_graph(seed=720, n=350, r=4, e=6000, shuffle=False)
    layer, x = _layer(g, 4, 64, 64, self_loop=self_loop, bias=bias)
    g.to_(DEV)
    out_f, out_t = _both(g, layer, x, calls)
    g.cpu_()
    assert torch.equal(out_f, out_t)


@pytest.mark.parametrize("bias", [True, False])
def test_bit_identity_input_width_outside_the_fused_self_loop(bias, monkeypatch):
    """K = 256 is outside rows_linear_bias_ok: there is no self-loop buffer to add into, the aggregation adds into zeros and the
    self-loop product and the bias follow in rows_add_bias, as in the training forward."""
    import het_amd.kernels as k
    assert not k.rows_linear_bias_ok(256, 64)
    calls = _count_calls(monkeypatch)
    g = random_graph(seed=721, n=350, r=4, e=6000, shuffle=False)
    layer, x = _layer(g, 4, 256, 64, mulfirst=True, bias=bias)
    g.to_(DEV)
    out_f, out_t = _both(g, layer, x, calls)
    ref = _oracle(g.get_separate_coo_original(), layer, x, g.get_num_nodes())
    g.cpu_()
    assert torch.equal(out_f, out_t)
    assert_close(out_f, ref, what="out")


def test_empty_relation_and_nodes_without_in_edges(monkeypatch):
    """random_graph leaves relation 1 empty; few edges on many nodes leave destinations without in-edges, whose rows are the
    self-loop product + bias exactly (the aggregation never touches them)."""
    import het_amd.kernels as k
    calls = _count_calls(monkeypatch)
    g = random_graph(seed=722, n=2000, r=5, e=1500, shuffle=False)
    s = g.get_separate_coo_original()
    assert int((s["rel_ptrs"][1:] == s["rel_ptrs"][:-1]).sum()) >= 1
    no_in = torch.ones(g.get_num_nodes(), dtype=torch.bool)
    no_in[s["col_indices"]] = False
    assert int(no_in.sum()) > 100
    layer, x = _layer(g, 4, 64, 64)
    g.to_(DEV)
    out_f, out_t = _both(g, layer, x, calls)
    ref = _oracle(g.get_separate_coo_original(), layer, x, g.get_num_nodes())
    g.cpu_()
    assert torch.equal(out_f, out_t)
    offs = torch.tensor([0, x.shape[0]], dtype=torch.int64, device=DEV)
    loop_bias = k.rows_linear_bias(offs, x, layer.loop_weight.detach().contiguous(), layer.h_bias.detach().contiguous())
    assert torch.equal(out_f[no_in.to(DEV)], loop_bias[no_in.to(DEV)])
    assert_close(out_f, ref, what="out")


@pytest.mark.parametrize("R,H,D", [(5, 4, 16), (5, 2, 32), (9, 4, 16)])
def test_bit_identity_ladder_graph_with_hubs(R, H, D, monkeypatch):
    """Degrees on both sides of HET_RGAT_HUB_MIN (256): the pack-form launch, the hub items and the hub finish all run."""
    calls = _count_calls(monkeypatch)
    g = ladder_graph(R=R, seed=3, shuffle=False)
    indeg = torch.bincount(g.get_separate_coo_original()["col_indices"])
    assert int((indeg > 256).sum()) >= 2 and int(((indeg > 0) & (indeg <= 256)).sum()) >= 2
    layer, x = _layer(g, H, 64, H * D, mulfirst=True)
    g.to_(DEV)
    out_f, out_t = _both(g, layer, x, calls)
    ref = _oracle(g.get_separate_coo_original(), layer, x, g.get_num_nodes())
    g.cpu_()
    assert torch.equal(out_f, out_t)
    assert_close(out_f, ref, what="out")


@pytest.mark.parametrize("self_loop", [True, False])
def test_bit_identity_sampled_block(self_loop, monkeypatch):
    """A block: the destinations are the first num_dst nodes, only their rows come back."""
    from het_amd.graph import HetGraph
    from het_amd.synth import IntegratedCOO
    calls = _count_calls(monkeypatch)
    gen = torch.Generator().manual_seed(5)
    N, nd, R, E = 900, 200, 4, 7000
    rel = torch.sort(torch.randint(0, R, (E,), generator=gen)).values
    coo = IntegratedCOO(N, R, torch.tensor([0, N]), torch.randint(0, N, (E,), generator=gen), torch.randint(0, nd, (E,), generator=gen),
                        rel, torch.arange(E))
    g = HetGraph.from_integrated_coo(coo)
    layer, x = _layer(g, 4, 64, 64, self_loop=self_loop)
    g.to_(DEV)
    out_f, out_t = _both(g, layer, x, calls, num_dst=nd)
    ref = _oracle(g.get_separate_coo_original(), layer, x, N, nd) if self_loop else None
    g.cpu_()
    assert out_f.shape == (nd, 64) and torch.equal(out_f, out_t)
    if ref is not None:  # (the oracle's self-loop runs on every node: its first nd rows are the block's)
        assert_close(out_f, ref, what="out")


def test_no_edges(monkeypatch):
    """E == 0: the layer is its self-loop + bias on either path (the single-node layer needs edges; the composition runs)."""
    from het_amd.graph import HetGraph
    from het_amd.synth import IntegratedCOO
    calls = _count_calls(monkeypatch)
    e = torch.zeros(0, dtype=torch.int64)
    g = HetGraph.from_integrated_coo(IntegratedCOO(50, 3, torch.tensor([0, 50]), e, e.clone(), e.clone(), e.clone()))
    layer, x = _layer(g, 4, 64, 64)
    g.to_(DEV)
    with torch.no_grad():
        out_f = layer(g, x)
    out_t = layer(g, x).detach()
    g.cpu_()
    assert calls["forward_only"] == 0
    assert torch.equal(out_f, out_t)
    assert_close(out_f, x.detach().cpu().double() @ layer.loop_weight.detach().cpu().double() + layer.h_bias.detach().cpu().double(), what="out")


@pytest.mark.parametrize("case", ["mag", "random", "mulfirst_off"])
def test_forward_only_matches_the_fp64_oracle(case, monkeypatch):
    """Bit-identity alone would pass if both paths were wrong together."""
    from het_amd.backend import rgat_fused_layer as FL
    calls = _count_calls(monkeypatch)
    if case == "mulfirst_off":
        monkeypatch.setattr(FL, "LITERAL_ER", True)
    g = mag_graph() if case == "mag" else random_graph(seed=730, n=500, r=5, e=12000, shuffle=False)
    layer, x = _layer(g, 4, 64, 64, mulfirst=case != "mulfirst_off")
    ref = _oracle(g.get_separate_coo_original(), layer, x, g.get_num_nodes())
    g.to_(DEV)
    with torch.no_grad():
        out = layer(g, x)
    g.cpu_()
    assert calls == {"forward_only": 1, "training": 0}
    assert_close(out, ref, what="out")


def _peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    return peak, out


def _memory_case(g, monkeypatch, H=4, X=64):
    """Peak memory of one forward-only call against one training forward under no_grad (HET_RGAT_FORWARD_ONLY=0), groupings warm.
    The training forward allocates ret [N,H,D] and q_rows [S_col,H,D] (and lse, q_sum, q_ref, a larger workspace) that the
    forward-only one does not: at least 4 X (N + S_col) bytes less, minus 1 MiB of allocator rounding -- from the tensor list."""
    from het_amd.backend import rgat_fused_layer as FL
    calls = _count_calls(monkeypatch)
    N = g.get_num_nodes()
    layer, x = _layer(g, H, 64, X, mulfirst=True)

    def run():
        with torch.no_grad():
            return layer(g, x)

    monkeypatch.setattr(FL, "FORWARD_ONLY", False)
    run()  # warm-up: unique lists, groupings, hub lists
    monkeypatch.setattr(FL, "FORWARD_ONLY", True)
    run()
    S_col = g.get_separate_unique_node_indices_single_sided()["node_indices_col"].numel()
    before = dict(calls)
    p_f, out_f = _peak_of(run)
    assert calls["forward_only"] == before["forward_only"] + 1 and calls["training"] == before["training"]
    monkeypatch.setattr(FL, "FORWARD_ONLY", False)
    p_t, out_t = _peak_of(run)
    assert calls["training"] == before["training"] + 1
    bound = 4 * X * (N + S_col) - 2 ** 20
    print(f"peak memory of one forward: forward-only {p_f / 2**20:.1f} MiB, training {p_t / 2**20:.1f} MiB, "
          f"difference {(p_t - p_f) / 2**20:.1f} MiB, required {bound / 2**20:.1f} MiB (N {N}, S_col {S_col})")
    assert torch.equal(out_f, out_t)
    assert p_t - p_f >= bound, (p_f, p_t, bound)


def test_forward_only_allocates_no_ret_and_no_run_sums(monkeypatch):
    from het_amd.graph import HetGraph
    from het_amd.synth import make_random
    g = HetGraph.from_integrated_coo(make_random(200000, 4, 2000000, seed=41))
    g.to_(DEV)
    _memory_case(g, monkeypatch)
    g.cpu_()


@pytest.mark.parametrize("case", ["op_by_op", "per_edge", "shape"])
def test_fallbacks_keep_working_under_no_grad(case, monkeypatch):
    """Calls the forward-only path does not cover run what they ran before: same output as with gradients on, no call to the new
    entry."""
    from het_amd.backend import rgat_fused_layer as FL
    calls = _count_calls(monkeypatch)
    H, X = (8, 64) if case == "shape" else (4, 64)  # heads of 8 floats: outside rgat_runs_shape_ok
    if case == "op_by_op":
        monkeypatch.setattr(FL, "rgat_layer_fused_ok", lambda *a, **k: False)
    if case == "per_edge":
        monkeypatch.setattr(FL, "PER_EDGE", True)
    g = random_graph(seed=740, n=300, r=4, e=5000, shuffle=False)
    layer, x = _layer(g, H, 64, X)
    ref = _oracle(g.get_separate_coo_original(), layer, x, g.get_num_nodes())
    g.to_(DEV)
    with torch.no_grad():
        out_n = layer(g, x)
    out_g = layer(g, x).detach()
    g.cpu_()
    assert calls["forward_only"] == 0
    assert torch.equal(out_n, out_g)
    assert_close(out_n, ref, what="out")


def test_full_size_bit_identity_and_memory(monkeypatch):
    """ogbn-mag shape (built as tests/test_gpu_fullsize.py builds it), feat 64, 4 heads."""
    from het_amd.graph import HetGraph
    from het_amd.synth import make_mag_like
    coo = make_mag_like(scale=1.0)
    for f in ("row", "col", "rel", "eids", "node_type_offsets"):
        setattr(coo, f, getattr(coo, f).to(DEV))
    g = HetGraph.from_integrated_coo(coo, full=True)
    del coo
    _memory_case(g, monkeypatch)  # (asserts torch.equal of the two outputs too)


def test_train_inference_mode(tmp_path):
    from het_amd import train
    log = tmp_path / "log.json"
    res = train.main(["--model", "rgat", "-d", "mag", "--scale", "0.002", "--full_graph_training", "--n_infeat", "64", "--num_classes", "64",
                      "--num_heads", "4", "--n_epochs", "6", "--dropout", "0.0", "--inference", "--logfile_enabled", "--logfilename", str(log)])
    assert res["mode"] == "inference" and res["mean_backward_ms"] == 0 and res["mean_forward_ms"] > 0
    assert json.loads(log.read_text().splitlines()[-1])["mode"] == "inference"
