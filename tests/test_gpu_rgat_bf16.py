"""The RGAT layer's evaluation path with bf16 activations (het_amd/layers.py::HET_RGATLayer, backend/rgat_fused_layer.py:
_forward_only_bf16, csrc/gat_compact.hip: the _fwd_bf16 kernels): values against the staged fp64 reference of the precision contract
(tests/_rgat_bf16_ref.py, validated on the CPU in tests/test_rgat_bf16_ref.py), which calls take the path, validation, memory.

The value bound: every element |out - ref| <= 2^-8 |ref| + A max|ref|.  2^-8 |ref| is the output's own rounding (half a bf16 unit)
and as much again for a value next to a rounding boundary.  A covers what the ORDER of the fp32 sums does to a result with bf16
roundings inside it: an intermediate that lands on the other side of a boundary moves one feat_c or h element by a whole bf16 unit,
whatever the size of the output element it feeds.  It is measured, not guessed: the staged reference evaluated on the CPU in fp32
against the same in fp64, on the cases below, needs an absolute term of 1.156e-3 (worst case shape_H8_D16_R5; per case:
tests/test_rgat_bf16_ref.py::test_abs_term_measurement_runs prints them); A is 4 x that -- the GPU's summation order differs from
both CPU orders -- and not below RGCN's 1e-5."""
import pytest
import torch

from tests import _rgat_bf16_ref as REF

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
A = 4.63e-3  # 4 x 1.156e-3 (see above)


def _count_calls(monkeypatch):
    import het_amd.kernels as k
    calls = {"bf16": 0, "forward_only": 0, "training": 0}

    def wrap(key, fn):
        def f(*a, **kw):
            calls[key] += 1
            return fn(*a, **kw)
        return f

    monkeypatch.setattr(k, "rgat_aggregate_compact_forward_bf16", wrap("bf16", k.rgat_aggregate_compact_forward_bf16))
    monkeypatch.setattr(k, "rgat_aggregate_compact_forward", wrap("forward_only", k.rgat_aggregate_compact_forward))
    monkeypatch.setattr(k, "rgat_aggregate_compact", wrap("training", k.rgat_aggregate_compact))
    return calls


def _check(name, out, ref):
    assert out.dtype == BF16 and out.shape == ref.shape, (out.dtype, out.shape, ref.shape)
    o, ref = out.detach().cpu().double(), ref.double()
    d = (o - ref).abs()
    bound = REF.REL * ref.abs() + A * float(ref.abs().max())
    print(f"{name}: rel L2 {float((o - ref).norm() / ref.norm()):.3e}, smallest absolute term that passes "
          f"{REF.smallest_abs_term(o, ref):.3e} (A = {A:.2e}), max excess over the bound {float((d - bound).max()):.3e}")
    assert bool((d <= bound).all()), f"{name}: {int((d > bound).sum())} elements outside 2^-8 |ref| + {A} max|ref|"


@pytest.mark.parametrize("name", REF.CASE_NAMES)
def test_values_against_the_staged_reference(name, monkeypatch):
    """Every row width of the run-sum form, el from the gathered row (D = 16, R <= 8) and gathered, default and folded flags,
    self-loop and bias on and off, a block (num_dst < N), hub destinations, a head padded from 8, input widths 100 and 32."""
    case = REF.CASES[REF.CASE_NAMES.index(name)]
    calls = _count_calls(monkeypatch)
    g, layer, x = REF.build_case(case)
    ref = REF.reference_of(case, g, layer, x)
    layer = layer.to(DEV)
    g.to_(DEV)
    with torch.no_grad():
        out = layer(g, x.to(DEV), case["nd"])
        torch.cuda.synchronize()
    g.cpu_()
    assert calls == {"bf16": 1, "forward_only": 0, "training": 0}, calls  # (the native path: the fallback is not what is measured)
    _check(name, out, ref)


def test_literal_er_switch_does_not_apply(monkeypatch):
    """HET_RGAT_LITERAL_ER=1: the bf16 path still takes er from the folded weight."""
    from het_amd.backend import rgat_fused_layer as FL
    monkeypatch.setattr(FL, "LITERAL_ER", True)
    case = REF.CASES[0]
    calls = _count_calls(monkeypatch)
    g, layer, x = REF.build_case(case)
    ref = REF.reference_of(case, g, layer, x)
    layer = layer.to(DEV)
    g.to_(DEV)
    with torch.no_grad():
        out = layer(g, x.to(DEV))
    g.cpu_()
    assert calls["bf16"] == 1
    _check("literal_er", out, ref)


def test_path_selection(monkeypatch):
    from het_amd.backend import rgat_fused_layer as FL
    calls = _count_calls(monkeypatch)
    case = REF._case("select", ("random", 700, 300, 4, 5000), 4, 64, 64)
    g, layer, x = REF.build_case(case)
    layer, xb = layer.to(DEV), x.to(DEV)
    g.to_(DEV)
    with torch.no_grad():  # bf16 under no_grad: one bf16 aggregate call, no fp32 call
        out = layer(g, xb)
    assert calls == {"bf16": 1, "forward_only": 0, "training": 0} and out.dtype == BF16 and out.grad_fn is None
    with torch.no_grad():  # a second identical call: the same bits
        out2 = layer(g, xb)
    assert calls["bf16"] == 2 and torch.equal(out, out2)
    with torch.no_grad():  # fp32 input: what it took before
        out32 = layer(g, xb.float())
    assert calls == {"bf16": 2, "forward_only": 1, "training": 0} and out32.dtype == torch.float32
    out32g = layer(g, xb.float())
    assert calls == {"bf16": 2, "forward_only": 1, "training": 1} and out32g.grad_fn is not None
    # bf16 with gradients required: the fp32 layer on x.float(), cast; bf16 output and bf16 x.grad
    xg = xb.clone().requires_grad_(True)
    outg = layer(g, xg)
    assert calls == {"bf16": 2, "forward_only": 1, "training": 2}
    assert outg.dtype == BF16 and torch.equal(outg.detach(), out32g.detach().to(BF16))
    outg.float().square().sum().backward()
    assert xg.grad is not None and xg.grad.dtype == BF16 and bool(torch.isfinite(xg.grad.float()).all())
    # HET_RGAT_FORWARD_ONLY=0 sends bf16 to the fallback too
    monkeypatch.setattr(FL, "FORWARD_ONLY", False)
    with torch.no_grad():
        out5 = layer(g, xb)
    assert calls == {"bf16": 2, "forward_only": 1, "training": 3}
    assert out5.dtype == BF16 and torch.equal(out5, out32.to(BF16))
    g.cpu_()


@pytest.mark.parametrize("case", ["per_edge", "op_by_op", "shape"])
def test_fallbacks(case, monkeypatch):
    """Calls outside the native path: the fp32 layer's output on x.float(), cast to bf16, bit for bit."""
    from het_amd.backend import rgat_fused_layer as FL
    calls = _count_calls(monkeypatch)
    H, X = (8, 64) if case == "shape" else (4, 64)  # heads of 8 floats on 8 heads: outside the run-sum form
    if case == "per_edge":
        monkeypatch.setattr(FL, "PER_EDGE", True)
    if case == "op_by_op":
        monkeypatch.setattr(FL, "rgat_layer_fused_ok", lambda *a, **k: False)
    g, layer, x = REF.build_case(REF._case(case, ("random", 740, 300, 4, 5000), H, 64, X))
    layer, xb = layer.to(DEV), x.to(DEV)
    g.to_(DEV)
    with torch.no_grad():
        out = layer(g, xb)
        ref = layer(g, xb.float()).to(BF16)
    g.cpu_()
    assert calls["bf16"] == 0 and out.dtype == BF16 and torch.equal(out, ref)


def test_nodes_without_in_edges_are_not_touched(monkeypatch):
    """Their rows are the self-loop product + bias, rounded once, exactly."""
    import het_amd.kernels as k
    calls = _count_calls(monkeypatch)
    case = REF._case("sparse", ("random", 722, 2000, 5, 1500), 4, 64, 64)
    g, layer, x = REF.build_case(case)
    ref = REF.reference_of(case, g, layer, x)
    no_in = torch.ones(g.get_num_nodes(), dtype=torch.bool)
    no_in[g.get_separate_coo_original()["col_indices"]] = False
    layer, xb = layer.to(DEV), x.to(DEV)
    g.to_(DEV)
    with torch.no_grad():
        out = layer(g, xb)
    g.cpu_()
    offs = torch.tensor([0, xb.shape[0]], dtype=torch.int64, device=DEV)
    h = k.rows_linear_bias_bf16(offs, xb, layer.loop_weight.detach().contiguous(), layer.h_bias.detach().contiguous())
    assert calls["bf16"] == 1 and torch.equal(out[no_in.to(DEV)], h[no_in.to(DEV)])
    _check("self-loop rows", h, REF.bf16_round(x.double() @ layer.loop_weight.detach().cpu().double() + layer.h_bias.detach().cpu().double()))
    _check("sparse", out, ref)


def test_validation_enqueues_nothing():
    """A misaligned or null h_inout, null groupings and an unsupported shape return the documented code; h_inout keeps its bits."""
    import het_amd.kernels as k
    from het_amd import _lib
    L = _lib.lib()
    g, layer, x = REF.build_case(REF._case("validate", ("random", 700, 300, 4, 5000), 4, 64, 64))
    g.to_(DEV)
    s = g.get_separate_coo_original()
    from het_amd.backend import rgat_fused_layer as FL
    if not FL._has_single_sided_lists(g):
        g.generate_separate_unique_node_indices_single_sided_for_each_etype()
    ss = g.get_separate_unique_node_indices_single_sided()
    srow, drow = FL._edge_rows(g, ss, True, s["rel_ptrs"], s["row_indices"], s["col_indices"], s["eids"])
    N, S_row, S_col = g.get_num_nodes(), ss["node_indices_row"].numel(), ss["node_indices_col"].numel()
    grp = k.rgat_compact_groupings(s["col_indices"], srow, drow, N, S_row, S_col, rel_ptrs=s["rel_ptrs"], drow_nodes=ss["node_indices_col"],
                                   drow_rel_ptrs=ss["rel_ptrs_col"])
    feat = torch.randn(S_row, 4, 16, device=DEV).to(BF16)
    er = torch.randn(S_col, 4, device=DEV)
    el = torch.randn(S_row, 4, device=DEV)
    h = torch.randn(N + 1, 64, device=DEV).to(BF16)
    keep = h.clone()
    ws = torch.empty(1 << 20, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()

    def call(by_dst, by_rel, hio, H=4, D=16, f=feat):
        return L.het_rgat_aggregate_compact_forward_bf16(by_dst, by_rel, 4, p(f), p(el), p(er), H, D, 0.2, hio, N, None, None, p(ws),
                                                         ws.numel() * 4, None)
    assert call(grp[0].handle, grp[3].handle, None) == 1 and b"h_inout" in L.het_last_error()
    assert call(grp[0].handle, grp[3].handle, h.data_ptr() + 8) == 1 and b"h_inout" in L.het_last_error()
    assert call(None, grp[3].handle, h.data_ptr()) == 1 and call(grp[0].handle, None, h.data_ptr()) == 1
    assert call(grp[0].handle, grp[3].handle, h.data_ptr(), H=8, D=8) == 3 and b"unsupported shape" in L.het_last_error()
    assert call(grp[0].handle, grp[3].handle, h.data_ptr(), H=3, D=16) == 3
    torch.cuda.synchronize()
    assert torch.equal(h, keep)
    assert call(grp[0].handle, grp[3].handle, h.data_ptr()) == 0  # ... and the same arguments, valid, run
    torch.cuda.synchronize()
    assert not torch.equal(h[:N], keep[:N]) and torch.equal(h[N:], keep[N:])
    g.cpu_()


def _peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, out


def test_bf16_call_halves_feat_c_and_h(monkeypatch):
    """The tensors the evaluation call allocates, feat_c [S_row,X] and h [nd,X], are bf16: the call's peak is at least
    0.9 (S_row X 2 + nd X 2) bytes below the fp32 call's (2 M edges on 200 K nodes: the allocator's 2 MiB blocks are well under the
    10 % slack)."""
    from het_amd.graph import HetGraph
    from het_amd.layers import HET_RGATLayer
    from het_amd.synth import make_random
    calls = _count_calls(monkeypatch)
    g = HetGraph.from_integrated_coo(make_random(200000, 4, 2000000, seed=41))
    N, X = g.get_num_nodes(), 64
    torch.manual_seed(0)
    layer = HET_RGATLayer(64, X, g.get_num_rels(), 4, self_loop=True, dropout=0.0).to(DEV)
    xb = (torch.randn(N, 64) * 0.5).to(BF16).to(DEV)
    x32 = xb.float()
    g.to_(DEV)

    def run(x):
        with torch.no_grad():
            return layer(g, x)

    run(x32), run(xb)  # warm-up: unique lists, groupings, hub lists
    S_row = g.get_separate_unique_node_indices_single_sided()["node_indices_row"].numel()
    p32, o32 = _peak_of(lambda: run(x32))
    p16, o16 = _peak_of(lambda: run(xb))
    g.cpu_()
    assert calls["bf16"] == 2 and calls["forward_only"] == 2
    need = 0.9 * (S_row * X * 2 + N * X * 2)
    print(f"peak memory of one evaluation call: fp32 {p32 / 2**20:.1f} MiB, bf16 {p16 / 2**20:.1f} MiB, difference "
          f"{(p32 - p16) / 2**20:.1f} MiB, required {need / 2**20:.1f} MiB (N {N}, S_row {S_row})")
    assert (S_row + N) * X * 2 * 0.1 > 2 * 2 ** 21, "graph too small for the allocator's granularity"
    assert p16 <= p32 - need, (p16, p32, need)
    d = (o16.float() - o32).abs()
    assert float(d.max()) <= 2.0 ** -6 * float(o32.abs().max())  # (sanity only: the value test is above)
