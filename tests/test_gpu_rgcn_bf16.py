"""The RGCN layer with bf16 activations (include/het_amd.h: het_rgcn_layer_forward_bf16 / _backward_bf16): bf16 input, output
and input gradient; fp32 parameters, parameter gradients, norm and sums.  Checked against oracle/layers.py::rgcn_layer in fp64
evaluated on the bf16-rounded input and output gradient (the fp32 weights taken exactly): the output and grad_x are rounded once,
so they sit within half a bf16 unit of the oracle plus the fp32 sums' error; grad_W and grad_bias are fp32 sums of exact products."""
import contextlib
import ctypes

import pytest
import torch

from oracle import layers as OL
from tests.util import random_graph

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16


def _check_bf16(name, a, ref):
    assert a.dtype == BF16, f"{name}: {a.dtype}"
    a, ref = a.detach().double().to(ref.device), ref.detach().double()
    d = (a - ref).abs()
    rel_l2 = float((a - ref).norm() / ref.norm().clamp_min(1e-300))
    bound = 2.0 ** -8 * ref.abs() + 1e-5 * float(ref.abs().max())
    worst = float((d - bound).max())
    print(f"{name}: rel L2 {rel_l2:.2e}, max excess over the elementwise bound {worst:.2e}")
    assert rel_l2 <= 3e-3, f"{name}: relative L2 error {rel_l2:.2e}"
    assert worst <= 0, f"{name}: {int((d > bound).sum())} elements outside 2^-8 |ref| + 1e-5 max|ref|"


def _check_f32(name, a, ref, tol=1e-5):
    assert a.dtype == torch.float32, f"{name}: {a.dtype}"
    a, ref = a.detach().double().to(ref.device), ref.detach().double()
    rel_l2 = float((a - ref).norm() / ref.norm().clamp_min(1e-300))
    print(f"{name}: rel L2 {rel_l2:.2e}")
    assert rel_l2 <= tol, f"{name}: relative L2 error {rel_l2:.2e}"


def _oracle(layer, s, N, xb, normv, gob, want_x=True, dev="cpu"):
    """fp64 oracle on the bf16-rounded x / gradout: (out, grad_x or None, grad_W, grad_bias)."""
    w64 = layer.weight.detach().double().to(dev).requires_grad_(True)
    b64 = layer.h_bias.detach().double().to(dev).requires_grad_(True)
    x64 = xb.detach().double().to(dev).requires_grad_(want_x)
    ref = OL.rgcn_layer(x64, w64, normv.double()[s["eids"].to(normv.device)].to(dev), s["rel_ptrs"].to(dev), s["row_indices"].to(dev),
                        s["col_indices"].to(dev), N, b64)
    grads = torch.autograd.grad(ref, ([x64] if want_x else []) + [w64, b64], gob.double().to(dev))
    return (ref.detach(),) + ((grads[0],) if want_x else (None,)) + tuple(grads[-2:])


def _layer(K, D, R, seed, **kw):
    from het_amd.layers import HET_EglRelGraphConv_EdgeParallel
    torch.manual_seed(seed)
    layer = HET_EglRelGraphConv_EdgeParallel(K, D, R, bias=True, **kw)
    with torch.no_grad():
        layer.h_bias.uniform_(-0.5, 0.5)  # (a non-zero bias: it is added inside the op before the single rounding)
    return layer


def _bf16_step(g, K, D, R, seed=1, want_x=True, ctx=contextlib.nullcontext, **kw):
    """One bf16 layer step on ``g`` against the oracle (on the CPU); returns the layer."""
    layer = _layer(K, D, R, seed, **kw)
    N, E = g.get_num_nodes(), g.get_num_edges()
    xb, norm, gob = torch.randn(N, K).to(BF16), torch.rand(E, 1), torch.randn(N, D).to(BF16)
    s = g.get_separate_coo_original()
    ref, gx_r, gw_r, gb_r = _oracle(layer, s, N, xb, norm, gob, want_x)
    g.to_(DEV)
    layer = layer.to(DEV)
    xd = xb.to(DEV).requires_grad_(want_x)
    with ctx():
        out = layer(g, xd, norm.to(DEV))
        assert out.dtype == BF16 and out.shape == (N, D)
        out.backward(gob.to(DEV))
    torch.cuda.synchronize()
    _check_bf16("out", out, ref)
    if want_x:
        _check_bf16("grad_x", xd.grad, gx_r)
    else:
        assert xd.grad is None
    _check_f32("grad_W", layer.weight.grad, gw_r)
    _check_f32("grad_bias", layer.h_bias.grad, gb_r)
    g.cpu_()
    return layer


def _count_calls(monkeypatch):
    import het_amd.kernels as k
    calls = {"fwd": 0, "bwd": 0, "want_x": []}
    fwd, bwd = k.rgcn_layer_forward_bf16, k.rgcn_layer_backward_bf16

    def f(*a, **kw):
        calls["fwd"] += 1
        return fwd(*a, **kw)

    def b(*a, **kw):
        calls["bwd"] += 1
        calls["want_x"].append(kw.get("want_x", True))
        return bwd(*a, **kw)
    monkeypatch.setattr(k, "rgcn_layer_forward_bf16", f)
    monkeypatch.setattr(k, "rgcn_layer_backward_bf16", b)
    return calls


@pytest.mark.parametrize("R", [1, 3, 7])
@pytest.mark.parametrize("K,D", [(32, 32), (32, 64), (64, 32), (64, 64)])
def test_rgcn_bf16_layer_matches_the_oracle(K, D, R, monkeypatch):
    """Graphs with an empty relation, nodes without in-edges, shuffled eids and a hub destination (the long-segment kernel): the
    bf16 kernels run (one forward and one backward call per step) and match the fp64 oracle."""
    import het_amd.kernels as k
    assert k.rgcn_layer_ok(R, K, D)
    calls = _count_calls(monkeypatch)
    for seed, n, e, shuffle in ((500, 97, 900, True), (501, 1500, 30000, False), (502, 4000, 2500, True)):
        _bf16_step(random_graph(seed=seed, n=n, r=R, e=e, shuffle=shuffle, empty_rel=R > 2), K, D, R)
    assert calls["fwd"] == 3 and calls["bwd"] == 3


def test_rgcn_bf16_output_width_padding(monkeypatch):
    """An output width below the kernels' (16 -> padded to 32): still the bf16 kernels, the bias zero-padded inside them."""
    calls = _count_calls(monkeypatch)
    _bf16_step(random_graph(seed=530, n=800, r=3, e=12000), 64, 16, 3, seed=2)
    assert calls["fwd"] == 1 and calls["bwd"] == 1


def test_rgcn_bf16_step_needs_no_fp32_copy_of_x(monkeypatch):
    """A mid-size graph: the bf16 step's peak memory (after a reset) is below the fp32 step's -- no [N, K] fp32 copy of x, a bf16
    output and input gradient -- and the bf16 entries run once each per step."""
    from het_amd.graph import HetGraph
    from het_amd.synth import make_random
    g = HetGraph.from_integrated_coo(make_random(200000, 4, 2000000, seed=41))
    g.to_(DEV)
    N, E = g.get_num_nodes(), g.get_num_edges()
    layer = _layer(64, 64, 4, 3).to(DEV)
    norm = torch.rand(E, 1, device=DEV)
    x32, go32 = torch.randn(N, 64, device=DEV), torch.randn(N, 64, device=DEV)
    xb, gob = x32.to(BF16), go32.to(BF16)

    def step(x, go):
        layer.zero_grad(set_to_none=True)
        xd = x.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = layer(g, xd, norm)
        out.backward(go)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        del out, xd
        return peak

    for _ in range(2):  # (groupings, maps and the sorted norm are built in the first steps)
        step(x32, go32), step(xb, gob)
    calls = _count_calls(monkeypatch)
    p32, p16 = step(x32, go32), step(xb, gob)
    print(f"peak memory of one step: fp32 {p32 / 2**20:.1f} MiB, bf16 {p16 / 2**20:.1f} MiB")
    assert calls["fwd"] == 1 and calls["bwd"] == 1
    assert p16 < p32 - N * 64 * 2, (p16, p32)
    g.cpu_()


@pytest.mark.parametrize("case", ["compact", "r8_64x64", "no_groupings"])
def test_rgcn_bf16_fallback_paths(case, monkeypatch):
    """Paths without bf16 kernels (compact_as_of_node_flag, 8 relations at 64 x 64 beyond the node pass's LDS, groupings off) run
    the fp32 layer on an upcast copy: bf16 outputs within the same bounds, no bf16 entry called."""
    from het_amd import plan
    calls = _count_calls(monkeypatch)
    R = 8 if case == "r8_64x64" else 3
    kw = dict(compact_as_of_node_flag=True, compact_direct_indexing_flag=True) if case == "compact" else {}
    ctx = (lambda: plan.forced(False)) if case == "no_groupings" else contextlib.nullcontext
    _bf16_step(random_graph(seed=540, n=1200, r=R, e=20000, empty_rel=True), 64, 64, R, ctx=ctx, **kw)
    assert calls["fwd"] == 0 and calls["bwd"] == 0


def test_rgcn_bf16_fixed_input_features(monkeypatch):
    """x without requires_grad: the backward asks for no input gradient (the gather pass is skipped), grad_W still matches."""
    calls = _count_calls(monkeypatch)
    _bf16_step(random_graph(seed=550, n=700, r=4, e=9000, shuffle=True), 64, 64, 4, want_x=False)
    assert calls["fwd"] == 1 and calls["want_x"] == [False]


def test_rgcn_bf16_validation_before_launch():
    """K = 48, a misaligned x and a grouping of the wrong R are refused with het_last_error text, before any launch."""
    from het_amd import _lib
    import het_amd.kernels as k
    g = random_graph(seed=560, n=300, r=3, e=3000)
    g.to_(DEV)
    s = g.get_separate_coo_original()
    N = g.get_num_nodes()
    gd, gs, dst_map, dst_order, src_map, src_order = k.rgcn_layer_plan(s["rel_ptrs"], s["eids"], s["row_indices"], s["col_indices"], N)
    L = _lib.lib()
    x = torch.zeros(N * 64 + 8, dtype=BF16, device=DEV)
    w, norm = torch.zeros(3, 64, 64, device=DEV), torch.ones(g.get_num_edges(), device=DEV)
    ssum = torch.empty(max(1, gd.num_segments), 64, device=DEV)
    ret = torch.empty(N, 64, dtype=BF16, device=DEV)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731
    strm = torch.cuda.current_stream().cuda_stream

    def fwd(R, K, xoff=0):
        return L.het_rgcn_layer_forward_bf16(gd.handle, R, N, p(x, xoff), p(w), p(norm), None, None, p(dst_map), p(dst_order), p(ssum),
                                             p(ret), K, 64, ctypes.c_void_p(strm))
    before = ret.clone()
    assert fwd(3, 48) == 1 and b"unsupported shape" in L.het_last_error()
    assert fwd(3, 64, xoff=2) == 1 and b"aligned" in L.het_last_error()
    assert fwd(4, 64) == 1 and b"grouping" in L.het_last_error()
    ws = torch.empty(int(L.het_rgcn_layer_backward_workspace(gs.num_segments, 64)) // 4 + 4, device=DEV)
    gw = torch.empty(3, 64, 64, device=DEV)
    rc = L.het_rgcn_layer_backward_bf16(gs.handle, gd.handle, 4, N, N, p(ssum), p(w), p(norm), None, p(x), p(src_map), p(src_order),
                                        p(ret), p(gw), None, 64, 64, p(ws), ws.numel() * 4, ctypes.c_void_p(strm))
    assert rc == 1 and b"het_rgcn_layer_backward_bf16" in L.het_last_error()
    torch.cuda.synchronize()
    assert torch.equal(ret.view(torch.int16), before.view(torch.int16))  # nothing was written
    g.cpu_()


def test_rgcn_bf16_two_sampled_layers(monkeypatch):
    """Two layers over NeighborSampler blocks (num_dst < N: the bias inside the op, the destination rows kept) with bf16 features,
    against the oracle applied block by block."""
    from het_amd.graph import HetGraph
    from het_amd.layers import HET_EglRelGraphConv_EdgeParallel
    from het_amd.sampling import NeighborSampler, run_blocks
    from het_amd.synth import make_random
    coo = make_random(3000, 4, 60000, seed=13)
    for f in ("row", "col", "rel", "eids", "node_type_offsets"):
        setattr(coo, f, getattr(coo, f).to(DEV))
    g = HetGraph.from_integrated_coo(coo, full=True)
    calls = _count_calls(monkeypatch)
    torch.manual_seed(6)
    layers = torch.nn.ModuleList([HET_EglRelGraphConv_EdgeParallel(64, 64, 4, activation=torch.relu),
                                  HET_EglRelGraphConv_EdgeParallel(64, 32, 4)])
    with torch.no_grad():
        for layer in layers:
            layer.h_bias.uniform_(-0.5, 0.5)
    layers = layers.to(DEV)
    x = torch.randn(coo.num_nodes, 64, device=DEV).to(BF16)
    norm = torch.rand(coo.num_edges, 1, device=DEV)
    seeds = torch.arange(0, 3000, 7, device=DEV)
    blocks = NeighborSampler(g, [8, 12], seed=3).sample_blocks(seeds)
    xin = x[blocks[0].nodes].detach().requires_grad_(True)
    kept = []

    def keep(module, args, o):  # (the first layer's output: its bf16 rows and, after the backward, their gradient)
        o.retain_grad()
        kept.append(o)
    hook = layers[0].register_forward_hook(keep)
    out = run_blocks(layers, blocks, xin, norm)
    hook.remove()
    assert out.dtype == BF16 and out.shape == (seeds.numel(), 32)
    gob = torch.randn(seeds.numel(), 32, device=DEV).to(BF16)
    out.backward(gob)
    torch.cuda.synchronize()
    assert calls["fwd"] == 2 and calls["bwd"] == 2
    h1 = kept[0]
    assert h1.dtype == BF16 and h1.grad.dtype == BF16
    # the oracle block by block in fp64, each on what the layer was given: its bf16 input rows and its bf16 output gradient
    for i, (layer, b, hin, hout, go, gin) in enumerate(((layers[0], blocks[0], xin, h1, h1.grad, xin.grad),
                                                         (layers[1], blocks[1], h1, out, gob, h1.grad))):
        s = {k_: v.cpu() for k_, v in b.graph.get_separate_coo_original().items()}
        w64 = layer.weight.detach().double().cpu().requires_grad_(True)
        b64 = layer.h_bias.detach().double().cpu().requires_grad_(True)
        h64 = hin.detach().double().cpu().requires_grad_(True)
        nb = norm[b.edge_ids].double().cpu()[s["eids"]]
        r = OL.rgcn_layer(h64, w64, nb, s["rel_ptrs"], s["row_indices"], s["col_indices"], b.graph.get_num_nodes(), b64)[: b.num_dst]
        if i == 0:
            r = torch.relu(r)
        gx_r, gw_r, gb_r = torch.autograd.grad(r, [h64, w64, b64], go.double().cpu())
        _check_bf16(f"layer {i} out", hout, r.detach())
        _check_bf16(f"layer {i} grad_x", gin, gx_r)
        _check_f32(f"layer {i} grad_W", layer.weight.grad, gw_r)
        _check_f32(f"layer {i} grad_bias", layer.h_bias.grad, gb_r)


def test_rgcn_bf16_layer_at_full_size(monkeypatch):
    """ogbn-mag size (make_mag_like, feat 64): the bf16 layer against the fp64 oracle evaluated on the GPU."""
    from het_amd.graph import HetGraph
    from het_amd.synth import make_mag_like
    coo = make_mag_like(scale=1.0)
    for f in ("row", "col", "rel", "eids", "node_type_offsets"):
        setattr(coo, f, getattr(coo, f).to(DEV))
    g = HetGraph.from_integrated_coo(coo, full=True)
    s = g.get_separate_coo_original()
    N, E, R = g.get_num_nodes(), g.get_num_edges(), g.get_num_rels()
    calls = _count_calls(monkeypatch)
    gen = torch.Generator(device=DEV).manual_seed(13)
    xb = (torch.randn(N, 64, device=DEV, generator=gen) * 0.3).to(BF16)
    norm = torch.rand(E, 1, device=DEV, generator=gen)
    gob = torch.randn(N, 64, device=DEV, generator=gen).to(BF16)
    layer = _layer(64, 64, R, 0).to(DEV)
    x = xb.clone().requires_grad_(True)
    out = layer(g, x, norm)
    out.backward(gob)
    torch.cuda.synchronize()
    assert calls["fwd"] == 1 and calls["bwd"] == 1
    w64 = layer.weight.detach().double().requires_grad_(True)
    b64 = layer.h_bias.detach().double().requires_grad_(True)
    x64 = xb.double().requires_grad_(True)
    ref = OL.rgcn_layer(x64, w64, norm.double(), s["rel_ptrs"], s["row_indices"], s["col_indices"], N, b64)
    ref.backward(gob.double())
    _check_bf16("out", out, ref)
    _check_bf16("grad_x", x.grad, x64.grad)
    _check_f32("grad_W", layer.weight.grad, w64.grad)
    _check_f32("grad_bias", layer.h_bias.grad, b64.grad)
