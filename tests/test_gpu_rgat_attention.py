"""HET_RGATLayer.forward(..., get_attention=True): the attention weights [E,H] in edge-id order, from the HIP pass on the evaluation
paths (csrc/gat_attention.hip) and from the torch composition everywhere else, against the fp64 reference of
tests/_rgat_attention_ref.py.

Bounds (tests/_rgat_attention_ref.py::measure, re-measured by tests/test_rgat_attention_abi.py): the largest deviation
|a - ref| / max(ref, 1e-4) of the reference evaluated in fp32 on the CPU from itself in fp64 over the cases of a family, times 4 (the
GPU sums in a third order):
    family   cases                                                    measured     bound
    fp32     VALUE_CASES (random / ladder graph x R 3, 5, 9 x 4 shapes)   1.11e-06   4.42e-06
    large    attn_l, attn_r x 400: max |el + er| ~ 130                    2.08e-05   8.29e-05
    bf16     BF16_CASES, the staged reference (rounded feat_c)            1.21e-04   4.81e-04
test_lse_out_of_the_library_call measures its own bounds the same way, on its own case (its docstring has the figures).
Every test in this file fails on a tree without get_attention or without the library entry -- test_layer_output_on_permuted_eids
because such a tree reads the graph's inverse indices by position (rgat_fused_layer._edge_rows)."""
import pytest
import torch

from tests import _rgat_attention_ref as A
from tests.util import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
MEASURED = {"fp32": 1.11e-6, "large": 2.08e-5, "bf16": 1.21e-4}
BOUND = {k: 4.0 * v for k, v in MEASURED.items()}


def _count_calls(monkeypatch):
    import het_amd.kernels as k
    calls = {"attention": 0, "forward_only": 0, "forward_only_bf16": 0, "training": 0}

    def wrap(name, key):
        real = getattr(k, name)

        def f(*a, **kw):
            calls[key] += 1
            return real(*a, **kw)
        monkeypatch.setattr(k, name, f)

    wrap("rgat_attention_compact", "attention")
    wrap("rgat_aggregate_compact_forward", "forward_only")
    wrap("rgat_aggregate_compact_forward_bf16", "forward_only_bf16")
    wrap("rgat_aggregate_compact", "training")
    return calls


def _record_library_calls(monkeypatch):
    from het_amd import _lib
    names = []
    real = _lib.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", call)
    return names


def _evaluate(g, layer, x, num_dst=None):
    """(h, attn) of an evaluation call, the graph and the layer moved to the GPU and the graph back."""
    g.to_(DEV)
    layer.to(DEV)
    with torch.no_grad():
        h, attn = layer(g, x.to(DEV), num_dst, get_attention=True)
    torch.cuda.synchronize()
    g.cpu_()
    return h, attn


def _check(attn, ref, family, what):
    E, H = ref.shape
    assert attn.shape == (E, H) and attn.dtype == torch.float32 and not attn.requires_grad and attn.grad_fn is None
    assert bool(torch.isfinite(attn).all()), what
    dev = A.deviation(attn, ref)
    print(f"{what}: max |a - ref| / max(ref, {A.FLOOR:g}) = {dev:.3e} (bound {BOUND[family]:.3e})")
    assert dev <= BOUND[family], (what, dev, BOUND[family])


@pytest.mark.parametrize("kind,R,H,D", A.VALUE_CASES)
def test_values_fp32(kind, R, H, D, monkeypatch):
    calls = _count_calls(monkeypatch)
    g, layer, x = A.build_case(kind, R, H, D)
    ref, feat = A.reference_of(g, layer, x)
    s = g.get_separate_coo_original()
    col, eids, N = s["col_indices"].clone(), s["eids"].clone(), g.get_num_nodes()
    h, attn = _evaluate(g, layer, x)
    assert calls["attention"] == 1 and calls["forward_only"] == 1 and calls["training"] == 0, calls
    _check(attn, ref, "fp32", f"{kind} R{R} H{H} D{D}")
    # per (destination, head) the weights sum to 1: each is off by at most BOUND of max(a, FLOOR)
    a64 = attn.detach().cpu().double()[eids]  # by position
    sums = torch.zeros(N, H, dtype=torch.float64).index_add(0, col, a64)
    deg = torch.bincount(col, minlength=N)
    assert float((sums[deg > 0] - 1).abs().max()) <= BOUND["fp32"] * (1 + float(deg.max()) * A.FLOOR)
    # the layer output rebuilt from the returned weights: index_add(attn . feat) + self-loop + bias, in fp64
    p = {n: t.detach().cpu().double() for n, t in layer.named_parameters()}
    out = torch.zeros(N, H, D, dtype=torch.float64).index_add(0, col, a64.unsqueeze(-1) * feat).view(N, H * D)
    out = out + x.double() @ p["loop_weight"] + p["h_bias"]
    assert_close(h, out, what="layer output from the returned weights")


@pytest.mark.parametrize("kind,R,H,D", [("random", 5, 4, 16), ("ladder", 5, 2, 32), ("ladder", 9, 8, 16)])
def test_rows_are_in_edge_id_order(kind, R, H, D, monkeypatch):
    """After permute_eids row i is the edge with id i, not the edge at position i."""
    calls = _count_calls(monkeypatch)
    g, layer, x = A.build_case(kind, R, H, D, shuffle=True)
    eids = g.get_separate_coo_original()["eids"].clone()
    assert not torch.equal(eids, torch.arange(eids.numel()))
    ref, _ = A.reference_of(g, layer, x)
    h, attn = _evaluate(g, layer, x)
    assert calls["attention"] == 1, calls
    _check(attn, ref, "fp32", f"shuffled {kind}")
    assert A.deviation(attn, ref[eids]) > 1e-2  # (by position it is another tensor: the check above could tell)


@pytest.mark.parametrize("kind,R,H,D", [("ladder", 5, 4, 16), ("random", 5, 2, 32), ("ladder", 9, 8, 16), ("random", 3, 1, 64)])
def test_phase_2_in_destination_order(kind, R, H, D, monkeypatch):
    """HET_RGAT_ATTN_ORDER=d (read at every call): phase 2 walks the grouping by destination and scatters the rows.  The same
    arithmetic on the same lse: the same bits as the default order, in edge-id order on a permuted graph too."""
    calls = _count_calls(monkeypatch)
    g, layer, x = A.build_case(kind, R, H, D, shuffle=True)
    ref, _ = A.reference_of(g, layer, x)
    g.to_(DEV)
    layer.to(DEV)
    xd = x.to(DEV)
    with torch.no_grad():
        monkeypatch.delenv("HET_RGAT_ATTN_ORDER", raising=False)
        _, a_pos = layer(g, xd, get_attention=True)
        monkeypatch.setenv("HET_RGAT_ATTN_ORDER", "d")
        _, a_dst = layer(g, xd, get_attention=True)
    torch.cuda.synchronize()
    g.cpu_()
    assert calls["attention"] == 2, calls
    _check(a_dst, ref, "fp32", f"destination order {kind} H{H}")
    assert torch.equal(a_dst, a_pos)


def test_sampled_block(monkeypatch):
    """num_dst < N: only the first rows of h come back, every edge's weights do -- those into destinations >= num_dst too."""
    calls = _count_calls(monkeypatch)
    g, layer, x = A.build_case("random", 5, 4, 16)
    ref, _ = A.reference_of(g, layer, x)
    nd = 100
    assert int((g.get_separate_coo_original()["col_indices"] >= nd).sum()) > 100
    h, attn = _evaluate(g, layer, x, num_dst=nd)
    assert calls["attention"] == 1 and h.shape == (nd, 64)
    _check(attn, ref, "fp32", "block")


def test_no_edges():
    from het_amd.graph import HetGraph
    from het_amd.layers import HET_RGATLayer
    from het_amd.synth import IntegratedCOO
    e = torch.zeros(0, dtype=torch.int64)
    g = HetGraph.from_integrated_coo(IntegratedCOO(50, 3, torch.tensor([0, 50]), e, e.clone(), e.clone(), e.clone()))
    layer = HET_RGATLayer(64, 64, 3, 4, self_loop=True, dropout=0.0)
    h, attn = _evaluate(g, layer, torch.randn(50, 64))
    assert attn.shape == (0, 4) and attn.dtype == torch.float32 and h.shape == (50, 64)


@pytest.mark.parametrize("kind,R,H,D", [("ladder", 5, 4, 16), ("random", 5, 2, 32)])
def test_large_scores(kind, R, H, D, monkeypatch):
    """|el + er| above 100: exp of the raw score overflows fp32; relative to the running maximum everything is finite."""
    calls = _count_calls(monkeypatch)
    g, layer, x = A.build_case(kind, R, H, D, scale=A.LARGE_SCALE)
    ref, _ = A.reference_of(g, layer, x)
    h, attn = _evaluate(g, layer, x)
    assert calls["attention"] == 1, calls
    zmax = A.max_abs_score(g, layer, x)
    assert zmax > 100, zmax
    assert bool(torch.isfinite(h).all())
    _check(attn, ref, "large", f"large scores {kind} (max |el + er| {zmax:.0f})")


def test_two_calls_give_the_same_bits(monkeypatch):
    """The ladder graph has destinations split over several work items: their records meet in a fixed order (no float atomics)."""
    calls = _count_calls(monkeypatch)
    g, layer, x = A.build_case("ladder", 5, 4, 16)
    g.to_(DEV)
    layer.to(DEV)
    xd = x.to(DEV)
    with torch.no_grad():
        h1, a1 = layer(g, xd, get_attention=True)
        h2, a2 = layer(g, xd, get_attention=True)
    g.cpu_()
    assert calls["attention"] == 2
    assert torch.equal(a1, a2) and torch.equal(h1, h2)


@pytest.mark.parametrize("kind,R,H,D", A.BF16_CASES)
def test_values_bf16(kind, R, H, D, monkeypatch):
    """A bf16 input: el is the dot of the ROUNDED feat_c row -- formed by the walk itself at (4, 16), R <= 8 (el_c is made for the
    attention pass then), gathered at (2, 32) -- and er the dot of the widened x with the folded weight."""
    import het_amd.kernels as k
    calls = _count_calls(monkeypatch)
    assert k.rgat_el_from_row(H, D, R) == (D == 16)
    g, layer, x = A.build_case(kind, R, H, D, bf16=True)
    ref, _ = A.reference_of(g, layer, x, staged=True)
    h, attn = _evaluate(g, layer, x)
    assert calls["attention"] == 1 and calls["forward_only_bf16"] == 1 and calls["forward_only"] == 0, calls
    assert h.dtype == torch.bfloat16
    _check(attn, ref, "bf16", f"bf16 {kind} H{H} D{D}")


def test_path_selection_and_no_side_effects(monkeypatch):
    """The native pass runs exactly on evaluation calls; without get_attention the sequence of library calls and the output are
    those of a call that does not name the argument, and with it the same sequence plus the one new entry at its end."""
    calls = _count_calls(monkeypatch)
    names = _record_library_calls(monkeypatch)
    g, layer, x = A.build_case("random", 5, 4, 16)
    ref, _ = A.reference_of(g, layer, x)
    g.to_(DEV)
    layer.to(DEV)
    xd = x.to(DEV)
    with torch.no_grad():
        layer(g, xd)  # warm-up: lists and groupings
        del names[:]
        h0 = layer(g, xd)
        seq0 = list(names)
        del names[:]
        h1 = layer(g, xd, None, get_attention=False)
        seq1 = list(names)
        del names[:]
        h2, attn = layer(g, xd, get_attention=True)
        seq2 = list(names)
    assert calls["attention"] == 1
    assert seq0 and seq1 == seq0 and torch.equal(h1, h0)
    assert seq2 == seq0 + ["het_rgat_attention_compact"] and torch.equal(h2, h0)
    # gradients on and parameters that train: the autograd node, and the composition for the weights
    h3, attn3 = layer(g, xd, get_attention=True)
    assert calls["attention"] == 1 and calls["training"] == 1 and h3.grad_fn is not None
    assert not attn3.requires_grad and attn3.grad_fn is None
    _check(attn3, ref, "fp32", "composition beside the autograd node")
    # ... nothing asks for a gradient: evaluation again
    for p in layer.parameters():
        p.requires_grad_(False)
    h4, attn4 = layer(g, xd, get_attention=True)
    assert calls["attention"] == 2 and torch.equal(attn4, attn) and torch.equal(h4, h0)
    g.cpu_()


def _lse_by_destination(z, col, num_nodes, slope=0.2):
    """lse [N,H] in the dtype of ``z`` [E,H] (scores by position): -inf where a destination has no in-edge."""
    H = z.shape[1]
    s = torch.where(z > 0, z, z * slope)
    m = torch.full((num_nodes, H), -float("inf"), dtype=z.dtype).scatter_reduce(0, col.unsqueeze(-1).expand(-1, H), s, "amax")
    den = torch.zeros(num_nodes, H, dtype=z.dtype).index_add(0, col, torch.exp(s - m[col]))
    return m + torch.log(den)


@pytest.mark.parametrize("H", [4, 8, 1])
def test_lse_out_of_the_library_call(H):
    """kernels.rgat_attention_compact with ``lse_out``: the log-sum-exp of every destination -- -inf where it has no in-edge (the
    fill launch), destinations split over several work items included (their records then sit at the start of the workspace) --
    and the same attn bits as the call that keeps lse in the workspace.  el_c / er_c are random fp32 tables, taken exactly by the
    fp64 reference.  Bounds, by the procedure of the header: 4 x the deviation of the same formulas evaluated in fp32 on the CPU,
    measured here on the case itself -- |lse - ref| / max(|ref|, 1) and |a - ref| / max(ref, 1e-4):
        H   lse measured  bound      attn measured  bound
        4   1.55e-07   6.20e-07      1.85e-06   7.40e-06
        8   1.69e-07   6.78e-07      1.68e-06   6.72e-06
        1   1.26e-07   5.02e-07      1.29e-06   5.17e-06
    (|el + er| up to 12, |lse| up to 14: an lse bound of 6e-07 is about 8 units in the last place there.)"""
    import het_amd.kernels as k
    g = A.build_graph("ladder", 5, shuffle=True)
    s, ss = g.get_separate_coo_original(), g.get_separate_unique_node_indices_single_sided()
    inv = g.get_separate_unique_node_indices_single_sided_inverse_idx()
    col, eids, N = s["col_indices"], s["eids"], g.get_num_nodes()
    srow, drow = inv["inverse_indices_row"][eids].contiguous(), inv["inverse_indices_col"][eids].contiguous()  # by position
    S_row, S_col = ss["node_indices_row"].numel(), ss["node_indices_col"].numel()
    gen = torch.Generator().manual_seed(77 + H)
    el, er = torch.randn(S_row, H, generator=gen) * 2, torch.randn(S_col, H, generator=gen) * 2
    z64 = el.double()[srow] + er.double()[drow]
    ref = _lse_by_destination(z64, col, N)
    deg = torch.bincount(col, minlength=N)
    assert int((deg == 0).sum()) >= 7 and int(deg.max()) > 256  # isolated nodes and split destinations
    rel = lambda t: float(((t.double() - ref)[deg > 0].abs() / ref[deg > 0].abs().clamp_min(1.0)).max())  # noqa: E731
    z32 = el[srow] + er[drow]
    lse32 = _lse_by_destination(z32, col, N)
    bound = 4.0 * rel(lse32)
    w64 = torch.exp(torch.where(z64 > 0, z64, z64 * 0.2) - ref[col])
    w32 = torch.exp(torch.where(z32 > 0, z32, z32 * 0.2) - lse32[col])
    aref = torch.empty_like(w64)
    aref[eids] = w64
    abound = 4.0 * A.deviation(w32, w64)
    print(f"lse_out H{H}: measured on the CPU in fp32: lse {bound / 4:.3e}, attn {abound / 4:.3e}")

    d = lambda t: t.to(DEV)  # noqa: E731
    cd, sd, dd, ed, eld, erd = d(col), d(srow), d(drow), d(eids), d(el), d(er)
    grp = k.rgat_compact_groupings(cd, sd, dd, N, S_row, S_col)
    lse = torch.full((N, H), 7.0, device=DEV)
    a1 = k.rgat_attention_compact(grp, eld, erd, 0.2, cd, sd, dd, ed, N, lse_out=lse)
    a0 = k.rgat_attention_compact(grp, eld, erd, 0.2, cd, sd, dd, ed, N)
    torch.cuda.synchronize()
    lse = lse.cpu()
    assert bool((lse[deg == 0] == -float("inf")).all())
    assert bool(torch.isfinite(lse[deg > 0]).all())
    dev = rel(lse)
    print(f"lse_out H{H}: max |lse - ref| / max(|ref|, 1) = {dev:.3e} (bound {bound:.3e})")
    assert dev <= bound, (dev, bound)
    assert torch.equal(a1, a0)
    adev = A.deviation(a1, aref)
    print(f"lse_out H{H}: max |a - ref| / max(ref, {A.FLOOR:g}) = {adev:.3e} (bound {abound:.3e})")
    assert a1.shape == aref.shape and bool(torch.isfinite(a1).all()) and adev <= abound, (adev, abound)


@pytest.mark.parametrize("kind", ["random", "ladder"])
def test_layer_output_on_permuted_eids(kind):
    """The rows of h when the edge ids are not the positions: the evaluation forward and the training forward and backward read the
    graph's inverse indices by edge id (rgat_fused_layer._edge_rows), against the fp64 reference and its autograd gradients."""
    from tests.util import rgat_min_abs_preactivation
    g, layer, x = A.build_case(kind, 5, 4, 16, shuffle=True)
    s = g.get_separate_coo_original()
    col, eids, N = s["col_indices"].clone(), s["eids"].clone(), g.get_num_nodes()
    assert not torch.equal(eids, torch.arange(eids.numel()))
    for _ in range(64):  # no (edge, head) on the leaky-ReLU kink (tests/util.py)
        if rgat_min_abs_preactivation(x, layer.conv_weights, layer.attn_l, layer.attn_r, s) >= 2e-6:
            break
        x = x + 1e-3 * torch.randn(x.shape)
    p = {n: t.detach().double().requires_grad_(True) for n, t in layer.named_parameters()}
    x64 = x.double().requires_grad_(True)
    a, feat = A.attention_reference(x64, p["conv_weights"], p["attn_l"], p["attn_r"], s["rel_ptrs"], s["row_indices"], col, eids, N)
    ref = torch.zeros(N, 4, 16, dtype=torch.float64).index_add(0, col, a[eids].unsqueeze(-1) * feat).view(N, 64)
    ref = ref + x64 @ p["loop_weight"] + p["h_bias"]
    wgt = torch.randn(N, 64, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    (ref * wgt).sum().backward()

    g.to_(DEV)
    layer.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    with torch.no_grad():
        h_eval = layer(g, xd)
    h_train = layer(g, xd)
    assert h_train.grad_fn is not None
    (h_train * wgt.to(DEV).float()).sum().backward()
    torch.cuda.synchronize()
    g.cpu_()
    assert_close(h_eval, ref, what="evaluation forward, permuted eids")
    assert_close(h_train, ref, what="training forward, permuted eids")
    assert_close(xd.grad, x64.grad, what="grad x, permuted eids")
    for n, t in layer.named_parameters():
        assert_close(t.grad, p[n].grad, what=f"grad {n}, permuted eids")


@pytest.mark.parametrize("case", ["requires_grad", "op_by_op", "per_edge"])
def test_fallbacks(case, monkeypatch):
    """Calls the evaluation kernels do not serve get the weights from the torch composition: same reference, same bound."""
    from het_amd.backend import rgat_fused_layer as FL
    calls = _count_calls(monkeypatch)
    g, layer, x = A.build_case("ladder", 5, 4, 16, shuffle=case == "op_by_op")
    ref, _ = A.reference_of(g, layer, x)
    if case == "op_by_op":
        layer.op_by_op = True  # HET_RGAT_FUSED=0
    if case == "per_edge":
        monkeypatch.setattr(FL, "PER_EDGE", True)
    g.to_(DEV)
    layer.to(DEV)
    if case == "requires_grad":
        h, attn = layer(g, x.to(DEV), get_attention=True)
        assert h.grad_fn is not None
    else:
        with torch.no_grad():
            h, attn = layer(g, x.to(DEV), get_attention=True)
    g.cpu_()
    assert calls["attention"] == 0, calls
    _check(attn, ref, "fp32", case)
