"""The RGAT layer's opt-in bf16 training step (het_amd/layers.py::HET_RGATLayer(bf16_training=True), backend/rgat_fused_layer.py:
RgatLayerBf16Function, csrc/gat_compact.hip and csrc/node_gemm.hip: the het_bf16 instances of the training kernels): values, which
calls take the path, fallbacks, repeatability, validation, memory.

Values: the project's criterion for bf16 training (tests/test_gpu_hgt_bf16.py::_layer_case).  For the output, grad_x and every
parameter gradient d_hip <= max(2 d_ref, 1e-5): d_ref the relative L2 distance of the staged fp64 emulation of the precision contract
(tests/_rgat_bf16_train_ref.py, validated on the CPU in tests/test_rgat_bf16_train_ref.py) to the fp64 oracle, d_hip that of the
layer, both measured in the same run on the same bf16 input and bf16 output gradient; 1e-5 is the fp32 floor of the RGCN and HGT
bf16 tests, for a gradient the roundings hardly reach (h_bias).

A whole-tensor distance cannot see one wrong row (a destination's output row off by 10 % moves it by 3e-3), so the output and grad_x are
also held row by row (tests/_rgat_bf16_train_ref.py::check_rowwise): with d[v] = ||a[v] - ref[v]|| / ||ref[v]||,
max_v d_hip[v] <= 2 max_v d_ref[v], d_ref from the same staged emulation in the same run.  max_v d_ref, measured on the CPU for all 21
cases (tests/test_bf16_rows_ref.py::test_rowwise_emulation_maxima prints them and caps them at 2.5e-2): 2.7e-3 .. 4.3e-3 for out;
2.2e-3 .. 2.6e-3 for grad_x with the self-loop term, 7.3e-3 .. 1.5e-2 without it, 1.9e-2 for the block (small rows)."""
import pytest
import torch

from tests import _rgat_bf16_ref as REF
from tests import _rgat_bf16_train_ref as TREF

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
NEW = ("rgat_aggregate_compact_bf16", "rgat_backward_compact_bf16", "rgat_node_backward_dx_bf16", "rows_dot1h_backward_dw_bf16")
FP32 = ("rgat_aggregate_compact", "rgat_backward_compact", "rgat_node_backward_dx")


def _count_calls(monkeypatch):
    import het_amd.kernels as k
    calls = {}

    def wrap(key, fn):
        def f(*a, **kw):
            calls[key] = calls.get(key, 0) + 1
            return fn(*a, **kw)
        return f

    for name in NEW + FP32:
        monkeypatch.setattr(k, name, wrap(name, getattr(k, name)))
    return calls


def _step(layer, g, x, go, nd=None):
    """One forward + backward: (out, x.grad, {parameter: grad})."""
    layer.zero_grad(set_to_none=True)
    xd = x.detach().clone().requires_grad_(True)
    out = layer(g, xd, nd)
    out.backward(go)
    torch.cuda.synchronize()
    return out.detach(), xd.grad, {n: p.grad for n, p in layer.named_parameters()}


def _assert_native(calls):
    assert calls.get("rgat_aggregate_compact_bf16") == 1 and calls.get("rgat_backward_compact_bf16") == 1, calls
    assert calls.get("rgat_node_backward_dx_bf16", 0) >= 1, calls
    assert not any(n in calls for n in FP32), calls


@pytest.mark.parametrize("name", TREF.CASE_NAMES)
def test_values_against_the_staged_emulation(name, monkeypatch):
    """el from the gathered row and el gathered, default and folded flags, self-loop and bias on and off, K = 32, a head padded from
    8, a block, and the ladder graph: hub destinations (runs of 257 / 513 in-edges over several work items), long (relation, source)
    segments (the atomic path) and destinations split over relations.  Whole-tensor distances for every tensor, and the row-wise
    criterion of the module docstring for the output and grad_x: wrong wiring between the passes (which er rows, which run sums reach
    the backward) shows in single rows."""
    case = TREF.CASES[TREF.CASE_NAMES.index(name)]
    g, layer, xb, gob = TREF.build_case(case)
    ref, emu = TREF.oracle_and_emulation(case, g, layer, xb, gob)
    calls = _count_calls(monkeypatch)
    layer = layer.to(DEV)
    g.to_(DEV)
    out, gx, pg = _step(layer, g, xb.to(DEV), gob.to(DEV), case["nd"])
    g.cpu_()
    _assert_native(calls)
    assert out.dtype == BF16 and gx.dtype == BF16 and out.shape == ref[0].shape and gx.shape == xb.shape
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(gx.float()).all())
    got = [out, gx] + [pg.get(n) for n in TREF.PARAMS]
    bad = []
    for n, a, r, e in zip(TREF.NAMES, got, ref, emu):
        assert (a is None) == (r is None), n
        if a is None:
            continue
        if n not in ("out", "grad_x"):
            assert a.dtype == torch.float32 and a.shape == r.shape, n
        d_ref, d_hip = TREF.rel_l2(e, r), TREF.rel_l2(a, r)
        print(f"{name} {n}: d_ref {d_ref:.3e} d_hip {d_hip:.3e}")
        if not d_hip <= max(2 * d_ref, 1e-5):
            bad.append((n, d_ref, d_hip))
    assert not bad, bad
    for n, a, r, e in zip(TREF.NAMES[:2], got[:2], ref[:2], emu[:2]):
        TREF.check_rowwise(f"{name} {n}", a, r, e)


def test_keyword_off_keeps_the_fp32_training_call(monkeypatch):
    """The same step on a layer built without the keyword: the fp32 entries and none of the new ones; its output is the fp32 layer's
    on x.float(), cast, bit for bit."""
    case = TREF.CASES[0]
    g, layer, xb, gob = TREF.build_case(case, bf16_training=False)
    calls = _count_calls(monkeypatch)
    layer = layer.to(DEV)
    g.to_(DEV)
    out, gx, _ = _step(layer, g, xb.to(DEV), gob.to(DEV))
    assert calls.get("rgat_aggregate_compact") == 1 and calls.get("rgat_backward_compact") == 1, calls
    assert calls.get("rgat_node_backward_dx", 0) >= 1 and not any(n in calls for n in NEW), calls
    ref = layer(g, xb.to(DEV).float().requires_grad_(True)).detach().to(BF16)
    g.cpu_()
    assert out.dtype == BF16 and gx.dtype == BF16 and torch.equal(out, ref)


def test_evaluation_and_fp32_inputs_are_unchanged_by_the_keyword(monkeypatch):
    """With the keyword on: a no_grad bf16 call is the evaluation path's output bit for bit -- and so is the training forward --, an
    fp32 input takes the fp32 training call."""
    case = TREF.CASES[0]
    g, layer, xb, gob = TREF.build_case(case)
    g2, layer_off, _, _ = TREF.build_case(case, bf16_training=False)
    layer_off.load_state_dict(layer.state_dict())
    layer, layer_off, xd = layer.to(DEV), layer_off.to(DEV), xb.to(DEV)
    g.to_(DEV)
    calls = _count_calls(monkeypatch)
    with torch.no_grad():
        ev, ev_off = layer(g, xd), layer_off(g, xd)
    assert not calls and ev.dtype == BF16 and torch.equal(ev, ev_off)
    out, _, _ = _step(layer, g, xd, gob.to(DEV))
    _assert_native(calls)
    assert torch.equal(out, ev)  # (the training aggregation stores the rows the evaluation one stores)
    calls.clear()
    o32, g32, _ = _step(layer, g, xd.float(), gob.to(DEV).float())
    assert o32.dtype == torch.float32 and g32.dtype == torch.float32 and calls.get("rgat_aggregate_compact") == 1 and not any(n in calls for n in NEW)
    g.cpu_()


def test_parameters_alone_requiring_a_gradient_train_natively(monkeypatch):
    case = TREF.CASES[0]
    g, layer, xb, gob = TREF.build_case(case)
    calls = _count_calls(monkeypatch)
    layer = layer.to(DEV)
    g.to_(DEV)
    out = layer(g, xb.to(DEV))
    assert out.dtype == BF16 and out.grad_fn is not None
    out.backward(gob.to(DEV))
    torch.cuda.synchronize()
    g.cpu_()
    _assert_native(calls)
    assert all(p.grad is not None and p.grad.dtype == torch.float32 for p in layer.parameters())


@pytest.mark.parametrize("case", ["K100", "R9", "per_edge", "op_by_op"])
def test_fallbacks_with_the_keyword_on(case, monkeypatch):
    """Calls outside the coverage: the fp32 layer's output on x.float() cast to bf16, bit for bit; a bf16, finite x.grad; none of
    the new entries."""
    from het_amd.backend import rgat_fused_layer as FL
    K, R = (100 if case == "K100" else 64), (9 if case == "R9" else 4)  # (an input width of 100 pads to 128)
    if case == "per_edge":
        monkeypatch.setattr(FL, "PER_EDGE", True)
    if case == "op_by_op":
        monkeypatch.setattr(FL, "rgat_layer_fused_ok", lambda *a, **k: False)
    g, layer, xb, gob = TREF.build_case(REF._case(case, ("random", 740, 400, R, 9000), 4, K, 64))
    calls = _count_calls(monkeypatch)
    layer, xd = layer.to(DEV), xb.to(DEV)
    g.to_(DEV)
    out, gx, _ = _step(layer, g, xd, gob.to(DEV))
    ref = layer(g, xd.float().requires_grad_(True)).detach().to(BF16)
    g.cpu_()
    assert not any(n in calls for n in NEW), calls
    assert out.dtype == BF16 and torch.equal(out, ref)
    assert gx.dtype == BF16 and bool(torch.isfinite(gx.float()).all())


def test_rows_without_in_edges_are_the_rounded_self_loop_and_bias(monkeypatch):
    import het_amd.kernels as k
    case = REF._case("sparse", ("random", 722, 2000, 5, 1500), 4, 64, 64)
    g, layer, xb, gob = TREF.build_case(case)
    no_in = torch.ones(g.get_num_nodes(), dtype=torch.bool)
    no_in[g.get_separate_coo_original()["col_indices"]] = False
    assert int(no_in.sum()) > 100
    calls = _count_calls(monkeypatch)
    layer, xd = layer.to(DEV), xb.to(DEV)
    g.to_(DEV)
    out, _, _ = _step(layer, g, xd, gob.to(DEV))
    g.cpu_()
    _assert_native(calls)
    offs = torch.tensor([0, xd.shape[0]], dtype=torch.int64, device=DEV)
    h = k.rows_linear_bias_bf16(offs, xd, layer.loop_weight.detach().contiguous(), layer.h_bias.detach().contiguous())
    assert torch.equal(out[no_in.to(DEV)], h[no_in.to(DEV)])


def test_two_steps_give_the_same_bits(monkeypatch):
    """A graph without hub destinations and without long (relation, source) segments: the output and x.grad -- what the gather passes
    and the node-major pass store, no float atomics there -- are the same bits from step to step.  (The parameter gradients meet in
    the float atomics of the weight-gradient launches, as the fp32 step's do: equal to fp32 rounding.)"""
    case = TREF.CASES[0]
    g, layer, xb, gob = TREF.build_case(case)
    calls = _count_calls(monkeypatch)
    layer, xd, god = layer.to(DEV), xb.to(DEV), gob.to(DEV)
    g.to_(DEV)
    o1, g1, p1 = _step(layer, g, xd, god)
    p1 = {n: t.clone() for n, t in p1.items()}
    o2, g2, p2 = _step(layer, g, xd, god)
    g.cpu_()
    assert calls.get("rgat_aggregate_compact_bf16") == 2
    assert torch.equal(o1, o2) and torch.equal(g1, g2)
    for n in p1:
        assert TREF.rel_l2(p2[n], p1[n]) <= 1e-6, n


def _tables(H=4, D=16):
    """Groupings and tables of a small graph for direct calls of the entries."""
    import het_amd.kernels as k
    from het_amd.backend import rgat_fused_layer as FL
    g, _, _ = REF.build_case(REF._case("validate", ("random", 700, 300, 4, 5000), H, 64, H * D))
    g.to_(DEV)
    s = g.get_separate_coo_original()
    if not FL._has_single_sided_lists(g):
        g.generate_separate_unique_node_indices_single_sided_for_each_etype()
    ss = g.get_separate_unique_node_indices_single_sided()
    srow, drow = FL._edge_rows(g, ss, True, s["rel_ptrs"], s["row_indices"], s["col_indices"], s["eids"])
    N, S_row, S_col = g.get_num_nodes(), ss["node_indices_row"].numel(), ss["node_indices_col"].numel()
    grp = k.rgat_compact_groupings(s["col_indices"], srow, drow, N, S_row, S_col, rel_ptrs=s["rel_ptrs"], drow_nodes=ss["node_indices_col"],
                                   drow_rel_ptrs=ss["rel_ptrs_col"])
    t = dict(feat=torch.randn(S_row + 1, H, D, device=DEV).to(BF16), el=torch.randn(S_row, H, device=DEV), er=torch.randn(S_col, H, device=DEV),
             sm=torch.zeros(N, H, device=DEV), ret=torch.zeros(N + 1, H, D, device=DEV), h=torch.randn(N + 1, H * D, device=DEV).to(BF16))
    return g, ss, grp, t, (N, S_row, S_col)


def test_validation_enqueues_nothing():
    """The Python entries refuse fp32 rows and shapes that do not fit with HetError; the C entries refuse rows off their alignment
    (8 bytes for bf16 rows, 16 for fp32 tables) with HET_ERR_INVALID_ARG; h_inout, ret and grad_x keep their bits."""
    import het_amd.kernels as k
    from het_amd import _lib
    L = _lib.lib()
    g, ss, grp, t, (N, S_row, S_col) = _tables()
    feat, el, er, sm, ret, h = t["feat"][:S_row], t["el"], t["er"], t["sm"], t["ret"][:N], t["h"][:N]
    keep_h, keep_ret = t["h"].clone(), t["ret"].clone()
    Err = _lib.HetError
    with pytest.raises(Err, match="bfloat16"):  # fp32 rows
        k.rgat_aggregate_compact_bf16(grp, feat.float(), el, er, sm, ret, 0.2, h, 4)
    with pytest.raises(Err, match="bfloat16"):
        k.rgat_aggregate_compact_bf16(grp, feat, el, er, sm, ret, 0.2, h.float(), 4)
    with pytest.raises(Err, match="float32"):  # a bf16 table that must be fp32
        k.rgat_aggregate_compact_bf16(grp, feat, el.to(BF16), er, sm, ret, 0.2, h, 4)
    with pytest.raises(Err, match="do not fit"):  # shapes
        k.rgat_aggregate_compact_bf16(grp, feat, el[:-1], er, sm, ret, 0.2, h, 4)
    with pytest.raises(Err, match="do not fit"):
        k.rgat_aggregate_compact_bf16(grp, feat, el, er, sm, ret, 0.2, h[:, :32].contiguous(), 4)
    go, gf, ge = torch.randn(N, 4, 16, device=DEV).to(BF16), torch.empty(S_row, 4, 16, device=DEV), torch.empty(S_col, 4, device=DEV)
    runs = (torch.zeros(S_col, 4, 16, device=DEV), torch.zeros(S_col, 4, device=DEV), torch.zeros(S_col, 4, device=DEV))
    with pytest.raises(Err, match="bfloat16"):
        k.rgat_backward_compact_bf16(grp, feat, el, er, sm, ret, go.float(), gf, None, ge, 0.2, runs, ss["node_indices_col"])
    with pytest.raises(Err, match="do not fit"):
        k.rgat_backward_compact_bf16(grp, feat, el, er, sm, ret, go[:-1], gf, None, ge, 0.2, runs, ss["node_indices_col"])
    gx = torch.zeros(N, 64, device=DEV).to(BF16)
    Wt, maps = torch.randn(4, 4, 16, 64, device=DEV), torch.full((4, N), -1, dtype=torch.int32, device=DEV)
    with pytest.raises(Err, match="bfloat16"):
        k.rgat_node_backward_dx_bf16(0, N, N, None, None, gf.view(-1, 64), Wt, maps, None, None, None, gx.float())
    with pytest.raises(Err, match="do not fit"):
        k.rgat_node_backward_dx_bf16(0, N, N, None, None, gf.view(-1, 64), Wt, maps, None, None, None, gx[:, :32].contiguous())
    with pytest.raises(Err, match="bfloat16"):
        k.rows_dot1h_backward_dw_bf16(ss["rel_ptrs_col"], ss["node_indices_col"], torch.randn(N, 64, device=DEV), ge, torch.empty(4, 4, 64, device=DEV), False)
    # rows off their alignment, straight at the C entries
    ws = torch.empty(1 << 20, device=DEV)
    p = lambda x: None if x is None else x.data_ptr()

    def agg(f=p(feat), hio=p(h), r=p(ret)):
        return L.het_rgat_aggregate_compact_runs_bf16(grp[0].handle, grp[3].handle, 4, f, p(el), p(er), p(sm), r, N, 4, 16, 0.2, hio, N,
                                                      p(runs[0]), p(runs[1]), p(runs[2]), S_col, None, None, p(ws), ws.numel() * 4, None)
    assert agg(f=p(feat) + 4) == 1 and b"8-byte" in L.het_last_error()
    assert agg(hio=p(h) + 4) == 1 and b"8-byte" in L.het_last_error()
    assert agg(r=p(ret) + 8) == 1 and b"16-byte" in L.het_last_error()
    assert L.het_rgat_aggregate_compact_runs_bf16(grp[0].handle, grp[3].handle, 4, p(feat), p(el), p(er), p(sm), p(ret), N, 8, 8, 0.2, p(h), N,
                                                  p(runs[0]), p(runs[1]), p(runs[2]), S_col, None, None, p(ws), ws.numel() * 4, None) == 3

    def bwd(f=p(feat), gr=p(go), out=p(gf)):
        return L.het_rgat_backward_compact_runs_bf16(grp[1].handle, p(runs[0]), p(runs[1]), p(runs[2]), p(ss["node_indices_col"]), f, p(el), p(er),
                                                     p(sm), p(ret), gr, out, None, p(ge), None, None, 0, None, 0, N, S_row, S_col, 4, 16, 0.2,
                                                     None, p(ws), ws.numel() * 4, None)
    keep_gf = gf.fill_(7.0).clone()
    assert bwd(f=p(feat) + 4) == 1 and b"8-byte" in L.het_last_error()
    assert bwd(gr=p(go) + 4) == 1 and b"8-byte" in L.het_last_error()
    assert bwd(out=p(gf) + 8) == 1 and b"16-byte" in L.het_last_error()

    def dx(out=p(gx), rows=p(gf)):
        return L.het_rgat_node_backward_dx_bf16(0, N, N, N, 4, None, None, rows, p(Wt), p(maps), None, None, None, out, 4, 64, 16, None, None)
    assert dx(out=p(gx) + 4) == 1 and b"8-byte" in L.het_last_error()
    assert dx(rows=p(gf) + 8) == 1 and b"16-byte" in L.het_last_error()
    torch.cuda.synchronize()
    assert torch.equal(t["h"], keep_h) and torch.equal(t["ret"], keep_ret) and torch.equal(gf, keep_gf) and not bool(gx.float().any())
    assert agg() == 0  # ... and the same arguments, valid, run
    torch.cuda.synchronize()
    assert not torch.equal(t["h"][:N], keep_h[:N]) and torch.equal(t["h"][N:], keep_h[N:]) and torch.equal(t["ret"][N:], keep_ret[N:])
    g.cpu_()


def test_bf16_step_needs_no_fp32_copy_of_the_rows(monkeypatch):
    """The bf16 step's peak allocation above its baseline is below the fp32 step's: x, feat_c, h, the output gradient and grad_x at half
    size and nothing upcast.  A condition, not a measurement: an accidental .float() of a row tensor breaks it."""
    from het_amd.graph import HetGraph
    from het_amd.layers import HET_RGATLayer
    from het_amd.synth import make_random
    g = HetGraph.from_integrated_coo(make_random(200000, 4, 2000000, seed=41))
    N = g.get_num_nodes()
    torch.manual_seed(0)
    layer = HET_RGATLayer(64, 64, g.get_num_rels(), 4, self_loop=True, dropout=0.0, bf16_training=True).to(DEV)
    g.to_(DEV)
    x32, go32 = torch.randn(N, 64, device=DEV) * 0.5, torch.randn(N, 64, device=DEV)
    xb, gob = x32.to(BF16), go32.to(BF16)

    def step(x, go):
        layer.zero_grad(set_to_none=True)
        xd = x.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = layer(g, xd)
        out.backward(go)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        del out, xd
        return peak

    for _ in range(2):  # (unique lists, groupings, hub lists and node maps are built in the first steps)
        step(x32, go32), step(xb, gob)
    calls = _count_calls(monkeypatch)
    p32, p16 = step(x32, go32), step(xb, gob)
    g.cpu_()
    print(f"peak memory of one RGAT step: fp32 {p32 / 2**20:.1f} MiB, bf16 {p16 / 2**20:.1f} MiB")
    assert calls.get("rgat_aggregate_compact_bf16") == 1 and calls.get("rgat_backward_compact_bf16") == 1 and calls.get("rgat_aggregate_compact") == 1, calls
    assert p16 < p32, (p16, p32)


def test_train_driver_flag(monkeypatch):
    """python -m het_amd.train --bf16_training: bf16 features into layers built with the keyword; every step is a native one."""
    import math
    from het_amd import train
    calls = _count_calls(monkeypatch)
    args = ["--model", "rgat", "-d", "mag", "--scale", "0.002", "--full_graph_training", "--n_infeat", "64", "--num_classes", "64",
            "--num_heads", "4", "--n_epochs", "4", "--dropout", "0.0"]
    res = train.main(args + ["--bf16_training"])
    steps = 5 + 4  # (warm-up + epochs)
    assert res["activations"] == "bf16" and res["args"]["bf16_training"] is True and math.isfinite(res["final_loss"])
    assert calls.get("rgat_aggregate_compact_bf16") == steps and calls.get("rgat_backward_compact_bf16") == steps, calls
    assert not any(n in calls for n in FP32), calls
    calls.clear()
    res = train.main(args)  # without the flag: the log line it always had, the fp32 step
    assert "activations" not in res and "bf16_training" not in res["args"]
    assert calls.get("rgat_aggregate_compact") == steps and not any(n in calls for n in NEW), calls
    with pytest.raises(SystemExit):
        train.main(["--model", "rgcn", "-d", "mag", "--scale", "0.002", "--full_graph_training", "--bf16_training"])
