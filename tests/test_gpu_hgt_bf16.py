"""The fused HGT layer with bf16 activations (het_amd/layers.py::HET_HGTLayerHetero, backend/hgt_fused_layer.py, csrc/hgt_compact.hip):
op parity of the bf16 row kernels, layer parity measured against a staged emulation of the rounding points, memory, fallbacks,
validation, full size.  The references are in tests/_hgt_bf16_ref.py, validated on the CPU in
tests/test_hgt_bf16_abi.py."""
import pytest
import torch

from oracle import ops as O
from tests._hgt_bf16_ref import PARAMS, attention_rows_backward, oracle_and_emulation
from tests._hgt_bf16_ref import check_bf16 as _check_bf16
from tests.util import assert_close, mag_graph, random_graph, to64

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
CASES = [(8, 8, 300, 5000), (1, 64, 300, 5000), (4, 16, 40, 9000), (2, 8, 12, 9000), (4, 32, 300, 700),
         (1, 32, 30, 4000), (2, 32, 300, 3000), (1, 8, 300, 5000), (1, 8, 12, 9000)]  # tests/test_gpu_ops.py::test_hgt_compact_passes


def _op_inputs(g, H, D):
    s = g.get_separate_coo_original()
    inv = g.get_separate_unique_node_indices_single_sided_inverse_idx()
    S_row = g.get_separate_unique_node_indices_single_sided()["node_indices_row"].numel()
    N = g.get_num_nodes()
    srow = inv["inverse_indices_row"][s["eids"]].contiguous()  # row of every edge POSITION
    gen = torch.Generator().manual_seed(6)
    kv, q, go = torch.randn(S_row, 2, H, D, generator=gen) * 0.6, torch.randn(N, H, D, generator=gen) * 0.6, torch.randn(N, H, D, generator=gen)
    return srow, s["col_indices"], N, S_row, kv.to(BF16), q.to(BF16), go.to(BF16)


def _op_case(g, H, D):
    import het_amd.kernels as k
    srow, col, N, S_row, kvb, qb, gob = _op_inputs(g, H, D)
    X = H * D
    kv64, q64, go64 = to64(kvb), to64(qb), to64(gob)
    den, out_r = O.hgt_attention_rows(kv64, q64, srow, col, N)
    grp = k.hgt_compact_groupings(col.to(DEV), srow.to(DEV), N, S_row)
    kvd, qd = kvb.to(DEV), qb.to(DEV)
    lsum, out = torch.full((N, H), 7.0, device=DEV), torch.full((N, X), 7.0, device=DEV, dtype=BF16)
    k.hgt_aggregate_compact_bf16(grp, kvd, qd, lsum, out)
    has_in = (den > 0).any(1)
    # 1. forward: out rounded once from fp32 acc / sum -> twice the half-ulp of bf16; lsum is fp32
    if bool(has_in.any()):
        assert_close(lsum[has_in.to(DEV)], torch.log(den[has_in]), what="log-sum-exp")
        _check_bf16("out", out.view(N, H, D), out_r)
    else:
        assert out.dtype == BF16
    assert float(out[(~has_in).to(DEV)].float().abs().max() if bool((~has_in).any()) else 0.0) == 0.0  # no in-edges: exactly zero rows
    # 2. backward: fp32 results against the explicit fp64 evaluation that takes <gradout, out> from the stored, rounded out
    gkv_r, gq_r = attention_rows_backward(kv64, q64, go64, out.detach().cpu().double().view(N, H, D), srow, col)
    gkv, gq = torch.full((S_row, 2, H, D), float("nan"), device=DEV), torch.full((N, H, D), float("nan"), device=DEV)
    k.hgt_backward_compact_bf16(grp, kvd, qd, lsum, out, gob.to(DEV).view(N, X), gkv, gq)
    assert gkv.dtype == torch.float32 and gq.dtype == torch.float32
    assert_close(gq, gq_r, what="grad_q")
    assert_close(gkv, gkv_r, what="grad_kv")


@pytest.mark.parametrize("H,D,n,e", CASES)
def test_hgt_bf16_compact_passes(H, D, n, e):
    """het_hgt_aggregate_compact_bf16 / het_hgt_backward_compact_bf16 on the graphs of the fp32 op test (hub destinations split over
    work items, long source segments)."""
    _op_case(random_graph(seed=29, n=n, r=4, e=e), H, D)


def test_hgt_bf16_compact_passes_without_edges():
    """A graph without edges: out, lsum and both gradients are exactly zero (every output row is written)."""
    import het_amd.kernels as k
    N, S_row, H, D = 50, 5, 4, 16
    empty = torch.empty(0, dtype=torch.int64, device=DEV)
    grp = k.hgt_compact_groupings(empty, empty.clone(), N, S_row)
    kvd, qd = torch.randn(S_row, 2 * H * D, device=DEV).to(BF16), torch.randn(N, H * D, device=DEV).to(BF16)
    lsum, out = torch.full((N, H), 7.0, device=DEV), torch.full((N, H * D), 7.0, device=DEV, dtype=BF16)
    k.hgt_aggregate_compact_bf16(grp, kvd, qd, lsum, out)
    assert float(out.float().abs().max()) == 0.0 and float(lsum.abs().max()) == 0.0
    gkv, gq = torch.full((S_row, 2 * H * D), float("nan"), device=DEV), torch.full((N, H * D), float("nan"), device=DEV)
    k.hgt_backward_compact_bf16(grp, kvd, qd, lsum, out, torch.randn(N, H * D, device=DEV).to(BF16), gkv, gq)
    assert float(gkv.abs().max()) == 0.0 and float(gq.abs().max()) == 0.0


# ---- layer -------------------------------------------------------------------------------------------------------------------
BF16_WRAPPERS = ("hgt_aggregate_compact_bf16", "hgt_backward_compact_bf16", "rows_matmul_bf16", "rows_matmul_backward_dw_bf16",
                 "node_rows_matmul_sum_bf16")


def _count_calls(monkeypatch):
    import het_amd.kernels as k
    calls = {}

    def spy(name):
        real = getattr(k, name)

        def f(*a, **kw):
            calls[name] = calls.get(name, 0) + 1
            return real(*a, **kw)
        monkeypatch.setattr(k, name, f)
    for name in BF16_WRAPPERS + ("hgt_aggregate_compact", "hgt_backward_compact"):
        spy(name)
    return calls


def _new_layer(g, H, in_dim, out_dim, fused_attn=False, **kw):
    from het_amd.layers import HET_HGTLayerHetero
    torch.manual_seed(4)
    layer = HET_HGTLayerHetero(g.get_num_ntypes(), g.get_num_rels(), in_dim, out_dim, num_heads=H, dropout=0.0,
                               hgt_fused_attn_score_flag=fused_attn, **kw)
    with torch.no_grad():
        layer.relation_pri.uniform_(0.5, 1.5)
        layer.skip.uniform_(-1, 1)
    return layer


def _rel(a, ref):
    return float((a.detach().double().to(ref.device) - ref).norm() / ref.norm().clamp_min(1e-300))


def _layer_case(g, fused_attn, compact_dst, H, in_dim, out_dim, monkeypatch, native, dev="cpu", node_major=True):
    """d_hip <= 2 d_ref for the output, grad_h and every parameter gradient: d_ref the distance of the staged emulation
    (tests/_hgt_bf16_ref.py::staged_emulation, rounding at the points of the contract) to the fp64 oracle, d_hip that of the
    layer, both measured in this run on the same bf16-rounded h / output gradient.  Where d_ref < 1e-5 (a parameter gradient the
    rounding hardly reaches, e.g. relation_pri) the bound is max(2 d_ref, 1e-5): the fp32 floor tests/test_gpu_rgcn_bf16.py::_check_f32 uses."""
    from het_amd.backend import hgt_fused_layer
    monkeypatch.setattr(hgt_fused_layer, "COMPACT_DST_BELOW", 2.0 if compact_dst else 0.0)
    N = g.get_num_nodes()
    layer = _new_layer(g, H, in_dim, out_dim, fused_attn)
    hb, gob = (torch.randn(N, in_dim) * 0.5).to(BF16), torch.randn(N, out_dim).to(BF16)
    if dev != "cpu":
        g.to_(DEV)
    ref, emu = oracle_and_emulation(g, layer, hb, gob, H, fused_attn, dev=dev)
    calls = _count_calls(monkeypatch)
    g.to_(DEV)
    layer = layer.to(DEV)
    hd = hb.to(DEV).requires_grad_(True)
    out = layer(g, hd)
    out.backward(gob.to(DEV))
    torch.cuda.synchronize()
    if dev == "cpu":
        g.cpu_()
    assert out.dtype == BF16 and out.shape == (N, out_dim) and hd.grad.dtype == BF16
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(hd.grad.float()).all())
    if native:  # the bf16 kernels ran, the fp32 row kernels did not
        assert calls.get("hgt_aggregate_compact_bf16") == 1 and calls.get("hgt_backward_compact_bf16") == 1, calls
        assert "hgt_aggregate_compact" not in calls and "hgt_backward_compact" not in calls, calls
        assert calls.get("rows_matmul_bf16", 0) >= 4 and calls.get("rows_matmul_backward_dw_bf16", 0) == 3, calls
        assert (calls.get("node_rows_matmul_sum_bf16", 0) >= 1) == node_major, calls
    got = [out, hd.grad] + [getattr(layer, n).grad for n in PARAMS]
    bad = []
    for name, a, r, e in zip(["out", "grad_h"] + ["grad_" + n for n in PARAMS], got, ref, emu):
        if name.startswith("grad_") and name != "grad_h":
            assert a.dtype == torch.float32, name
        d_ref, d_hip = _rel(e, r), _rel(a, r)
        print(f"H={H} in={in_dim} out={out_dim} fused_attn={fused_attn} compact_dst={compact_dst} {name}: d_ref {d_ref:.3e} d_hip {d_hip:.3e}")
        if not d_hip <= max(2 * d_ref, 1e-5):
            bad.append((name, d_ref, d_hip))
    assert not bad, bad
    return out


MODES = [(False, True), (True, True), (False, False)]


@pytest.mark.parametrize("fused_attn,compact_dst", MODES)
@pytest.mark.parametrize("H,in_dim,out_dim", [(8, 64, 64), (1, 64, 64), (4, 64, 64), (2, 32, 64), (1, 32, 32),
                                              (8, 64, 32), (4, 16, 64)])  # (heads of 4 padded to 8; input width 16 padded to 32)
def test_hgt_bf16_layer_native(fused_attn, compact_dst, H, in_dim, out_dim, monkeypatch):
    _layer_case(mag_graph(1.5e-3), fused_attn, compact_dst, H, in_dim, out_dim, monkeypatch, native=True)


@pytest.mark.parametrize("fused_attn,compact_dst", MODES)
@pytest.mark.parametrize("H,in_dim,out_dim", [(2, 64, 10), (4, 100, 64), (4, 128, 128), (8, 64, 256)])
def test_hgt_bf16_layer_any_path(fused_attn, compact_dst, H, in_dim, out_dim, monkeypatch):
    """Head padding, input-width padding, 128-wide rows, two head groups: served by the fp32 path on an upcast copy."""
    _layer_case(mag_graph(1.5e-3), fused_attn, compact_dst, H, in_dim, out_dim, monkeypatch, native=False)


def _hub_graph():
    from het_amd.graph import HetGraph
    from het_amd.synth import IntegratedCOO
    gen = torch.Generator().manual_seed(4)
    N, E = 500, 6000
    col = torch.randint(0, 40, (E,), generator=gen)
    col[: E // 2] = 7  # hub: 3000 in-edges, split over work items
    row = torch.randint(0, N, (E,), generator=gen)
    rel = torch.sort(torch.randint(0, 2, (E,), generator=gen) * 2).values  # relations 0 and 2; relation 1 is empty
    return HetGraph.from_integrated_coo(IntegratedCOO(N, 3, torch.tensor([0, N]), row, col, rel, torch.randperm(E, generator=gen)))


@pytest.mark.parametrize("compact_dst", [True, False])
def test_hgt_bf16_layer_hub_destination_and_empty_relation(compact_dst, monkeypatch):
    out = _layer_case(_hub_graph(), False, compact_dst, 8, 64, 64, monkeypatch, native=True)
    assert float(out.detach()[40:].float().abs().max()) == 0.0  # destinations without in-edges


def test_hgt_bf16_layer_four_relations_per_type(monkeypatch):
    """More relations leaving one node type than the node-major input gradient keeps in LDS: still the bf16 kernels; the input
    gradient is added relation by relation in an fp32 buffer and rounded once."""
    _layer_case(random_graph(seed=31, n=600, r=4, e=9000, empty_rel=False, shuffle=False), False, True, 4, 64, 64, monkeypatch, native=True,
                node_major=False)  # (layers read the inverse indices by position: canonical eids)


def test_hgt_bf16_step_needs_no_fp32_copy_of_the_rows(monkeypatch):
    """The bf16 step's peak allocation above its baseline is below the fp32 step's: h, kv_c, q, new_h, the output and grad_h at
    half size and nothing upcast.  A condition, not a measurement: an accidental .float() of a row tensor breaks it."""
    from het_amd.graph import HetGraph
    from het_amd.synth import make_random
    g = HetGraph.from_integrated_coo(make_random(200000, 4, 2000000, seed=41))
    g.to_(DEV)
    N = g.get_num_nodes()
    layer = _new_layer(g, 8, 64, 64).to(DEV)
    h32, go32 = torch.randn(N, 64, device=DEV) * 0.5, torch.randn(N, 64, device=DEV)
    hb, gob = h32.to(BF16), go32.to(BF16)

    def step(h, go):
        layer.zero_grad(set_to_none=True)
        hd = h.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = layer(g, hd)
        out.backward(go)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        del out, hd
        return peak

    for _ in range(2):  # (groupings, lists and plans are built in the first steps)
        step(h32, go32), step(hb, gob)
    calls = _count_calls(monkeypatch)
    p32, p16 = step(h32, go32), step(hb, gob)
    print(f"peak memory of one HGT step: fp32 {p32 / 2**20:.1f} MiB, bf16 {p16 / 2**20:.1f} MiB")
    assert calls.get("hgt_aggregate_compact_bf16") == 1 and calls.get("hgt_backward_compact_bf16") == 1, calls
    assert p16 < p32, (p16, p32)
    g.cpu_()


def _fallback_step(layer, g, hb, gob, num_dst=None):
    outs = []
    for h in (hb.float(), hb):
        layer.zero_grad(set_to_none=True)
        hd = h.clone().requires_grad_(True)
        out = layer(g, hd) if num_dst is None else layer(g, hd, num_dst)
        out.backward(gob.to(out.dtype))
        outs.append((out.detach(), hd.grad, {n: getattr(layer, n).grad.clone() for n in PARAMS}))
    (o32, g32, p32), (o16, g16, p16) = outs
    _check_bf16("out", o16, o32)
    _check_bf16("grad_h", g16, g32)
    for n in PARAMS:
        assert p16[n].dtype == torch.float32, n
    return p32, p16


@pytest.mark.parametrize("case", ["fused_off", "weights_first", "sampled_block"])
def test_hgt_bf16_fallback_paths(case, monkeypatch):
    """Paths without bf16 kernels: fp32 on an upcast copy, one final rounding -- bf16 output and h.grad that agree with the fp32
    layer on h.float() to that rounding, fp32 parameter gradients.  (multiply_among_weights_first_flag has a composition of its
    own only where the fused path is off: the fused path computes the same function for either value of the flag.)"""
    from het_amd.backend import hgt_fused_layer
    calls = _count_calls(monkeypatch)
    if case == "sampled_block":
        from het_amd.graph import HetGraph
        from het_amd.sampling import NeighborSampler
        from het_amd.synth import make_mag_like
        coo = make_mag_like(scale=4e-4)
        for f in ("row", "col", "rel", "eids", "node_type_offsets"):
            setattr(coo, f, getattr(coo, f).cuda())
        full = HetGraph.from_integrated_coo(coo, full=True)
        gen = torch.Generator(device=DEV).manual_seed(1)
        seeds = torch.randperm(coo.num_nodes, device=DEV, generator=gen)[:40]
        b = NeighborSampler(full, [-1], by_type=True).sample_blocks(seeds)[0]
        g, num_dst = b.graph, b.num_dst
        assert g.graph_data["original"].get("node_segment_types") is not None
        layer = _new_layer(full, 4, 64, 64).to(DEV)
        n_in = b.nodes.numel()
    else:
        monkeypatch.setattr(hgt_fused_layer, "FUSED", False)
        g, num_dst = mag_graph(1.5e-3), None
        g.to_(DEV)
        H = 1 if case == "weights_first" else 4
        layer = _new_layer(g, H, 64, 64, multiply_among_weights_first_flag=case == "weights_first").to(DEV)
        n_in = g.get_num_nodes()
    hb = (torch.randn(n_in, 64, device=DEV) * 0.5).to(BF16)
    gob = torch.randn(n_in if num_dst is None else num_dst, 64, device=DEV).to(BF16)
    p32, p16 = _fallback_step(layer, g, hb, gob, num_dst)
    for n in PARAMS:  # (the gradient reaches the parameters through the same fp32 graph, from the bf16-rounded output gradient)
        assert _rel(p16[n], p32[n].double()) <= 1e-5, n
    assert not any(name in calls for name in BF16_WRAPPERS), calls


def test_hgt_bf16_validation_before_launch():
    """The bf16 entries refuse, with HetError and no launch: fp32 where bf16 rows are expected and the reverse, non-contiguous rows,
    an unsupported (H, D), a workspace that is too small or misaligned, swapped groupings."""
    import het_amd.kernels as k
    H, D = 2, 8
    srow, col, N, S_row, kvb, qb, gob = _op_inputs(random_graph(seed=29, n=12, r=4, e=9000), H, D)  # (hub destinations: a forward workspace)
    X = H * D
    assert S_row > N
    grp = k.hgt_compact_groupings(col.to(DEV), srow.to(DEV), N, S_row)
    kvd, qd, god = kvb.to(DEV), qb.to(DEV).view(N, X), gob.to(DEV).view(N, X)
    lsum, out = torch.zeros(N, H, device=DEV), torch.zeros(N, X, device=DEV, dtype=BF16)
    gkv, gq = torch.zeros(S_row, 2 * X, device=DEV), torch.zeros(N, X, device=DEV)
    err = k._lib.HetError
    with pytest.raises(err, match="expected contiguous bfloat16"):
        k.hgt_aggregate_compact_bf16(grp, kvd.float(), qd, lsum, out)
    with pytest.raises(err, match="expected contiguous float32"):
        k.hgt_aggregate_compact_bf16(grp, kvd, qd, lsum.to(BF16), out)
    with pytest.raises(err, match="expected contiguous float32"):
        k.hgt_aggregate_compact(grp, kvd, qd, lsum, out)  # (the fp32 entry refuses bf16 rows as before)
    with pytest.raises(err, match="expected contiguous float32"):
        k.hgt_backward_compact_bf16(grp, kvd, qd, lsum, out, god, gkv.to(BF16), gq)
    with pytest.raises(err, match="non-contiguous"):
        k.hgt_aggregate_compact_bf16(grp, kvd, torch.zeros(X, N, device=DEV, dtype=BF16).t(), lsum, out)
    with pytest.raises(err, match="unsupported shape"):
        k.hgt_aggregate_compact_bf16(grp, torch.zeros(S_row, 2 * 24, device=DEV, dtype=BF16), torch.zeros(N, 24, device=DEV, dtype=BF16),
                                     torch.zeros(N, 3, device=DEV), torch.zeros(N, 24, device=DEV, dtype=BF16))
    with pytest.raises(err, match="unsupported shape"):
        k.hgt_backward_compact_bf16(grp, torch.zeros(S_row, 2 * 24, device=DEV, dtype=BF16), torch.zeros(N, 24, device=DEV, dtype=BF16),
                                    torch.zeros(N, 3, device=DEV), torch.zeros(N, 24, device=DEV, dtype=BF16),
                                    torch.zeros(N, 24, device=DEV, dtype=BF16), torch.zeros(S_row, 48, device=DEV), torch.zeros(N, 24, device=DEV))
    need = int(k._lib.lib().het_hgt_aggregate_compact_workspace(grp[0].handle, H, D))
    assert need > 0
    big = torch.zeros(need // 4 + 8, device=DEV)
    with pytest.raises(err, match="workspace"):
        k.hgt_aggregate_compact_bf16(grp, kvd, qd, lsum, out, workspace=big[:need // 4 - 4])
    with pytest.raises(err, match="workspace"):
        k.hgt_aggregate_compact_bf16(grp, kvd, qd, lsum, out, workspace=big[1:])  # 4 bytes off a 16-byte boundary
    need_b = int(k._lib.lib().het_hgt_backward_compact_workspace(N, H))
    bigb = torch.zeros(need_b // 4 + 8, device=DEV)
    with pytest.raises(err, match="workspace"):
        k.hgt_backward_compact_bf16(grp, kvd, qd, lsum, out, god, gkv, gq, workspace=bigb[:need_b // 4 - 4])
    with pytest.raises(err, match="workspace"):
        k.hgt_backward_compact_bf16(grp, kvd, qd, lsum, out, god, gkv, gq, workspace=bigb[1:])
    with pytest.raises(err, match="by_dst"):
        k.hgt_aggregate_compact_bf16((grp[1], grp[0]), kvd, qd, lsum, out, workspace=big)
    with pytest.raises(err, match="by_dst"):
        k.hgt_backward_compact_bf16((grp[1], grp[0]), kvd, qd, lsum, out, god, gkv, gq)
    # the row products: wrong dtypes and shapes outside the matrix-core ones
    rp = torch.tensor([0, N], device=DEV)
    with pytest.raises(err, match="expected contiguous bfloat16"):
        k.rows_matmul_bf16(rp, None, None, torch.zeros(1, 1, 64, 64, device=DEV), torch.zeros(N, 64, device=DEV), torch.zeros(N, 64, device=DEV, dtype=BF16))
    with pytest.raises(err, match="K in"):
        k.rows_matmul_bf16(rp, None, None, torch.zeros(1, 1, 48, 64, device=DEV), torch.zeros(N, 48, device=DEV, dtype=BF16),
                           torch.zeros(N, 64, device=DEV, dtype=BF16))
    with pytest.raises(err, match="do not fit"):
        k.rows_matmul_bf16(rp, None, None, torch.zeros(1, 1, 64, 64, device=DEV), torch.zeros(N, 32, device=DEV, dtype=BF16),
                           torch.zeros(N, 64, device=DEV, dtype=BF16))
    with pytest.raises(err, match="K in"):
        k.rows_matmul_backward_dw_bf16(rp, None, torch.zeros(N, 128, device=DEV, dtype=BF16), torch.zeros(N, 64, device=DEV),
                                       torch.zeros(1, 1, 128, 64, device=DEV), False)
    torch.cuda.synchronize()


def test_hgt_bf16_layer_at_full_size(monkeypatch):
    """BASELINE.json configs[3] (ogbn-mag shape, feat 64, 8 heads) in bf16: d_hip <= 2 d_ref with the oracle and the staged emulation
    evaluated in fp64 on the GPU; finite everywhere; rows of nodes without in-edges zero."""
    from tests.test_gpu_fullsize import _full_graph
    g = _full_graph()
    out = _layer_case(g, False, True, 8, 64, 64, monkeypatch, native=True, dev=DEV)
    col = g.get_separate_coo_original()["col_indices"]
    has_in = torch.zeros(g.get_num_nodes(), dtype=torch.bool, device=DEV)
    has_in[col] = True
    assert float(out.detach()[~has_in].float().abs().max()) == 0.0
