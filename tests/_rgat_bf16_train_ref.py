"""References of tests/test_gpu_rgat_bf16_train.py that need no GPU: the staged fp64 emulation of the RGAT layer's bf16 TRAINING contract
(het_amd/backend/rgat_fused_layer.py: RgatLayerBf16Function) with gradients, the fp64 oracle beside it, and the cases the GPU value
test runs.  tests/test_rgat_bf16_train_ref.py validates the emulation against the oracle on the CPU.

The forward is tests/_rgat_bf16_ref.py::staged_reference, imported and not edited: while it runs, its rounding function is the
straight-through one of tests/_hgt_bf16_ref.py::_Round -- the value is rounded to bf16, the gradient passes unchanged -- at feat_c, at
the self-loop + bias rows h and at the output, which is where the contract rounds; on the way back the gradient of x is rounded once,
after every term of a node is summed.  Everything else (el_c from the rounded row, er_c from the folded weight, the softmax, every
sum and every parameter gradient) is not rounded."""
import contextlib

import torch

from tests import _rgat_bf16_ref as REF
from tests._hgt_bf16_ref import _Round

BF16 = torch.bfloat16
PARAMS = ("conv_weights", "attn_l", "attn_r", "loop_weight", "h_bias")
NAMES = ("out", "grad_x") + tuple("grad_" + n for n in PARAMS)


@contextlib.contextmanager
def _straight_through_rounding():
    """REF.staged_reference rounds with the module's bf16_round: a plain cast, whose autograd backward would round the GRADIENT too."""
    keep = REF.bf16_round
    REF.bf16_round = lambda t: _Round.apply(t, True, False)
    try:
        yield
    finally:
        REF.bf16_round = keep


def staged_emulation(x, p, rel_ptrs, row, col, num_nodes, gradout, slope=0.2, num_dst=None, rounding=True):
    """(out, grad_x, grad of every name of PARAMS or None) of the staged layer in the dtype of ``x`` (fp64) for the output gradient
    ``gradout``; ``p``: name -> parameter (missing: the layer has none).  ``rounding`` False: no rounding anywhere."""
    xr = x.detach().clone().requires_grad_(True)
    q = {n: t.detach().clone().requires_grad_(True) for n, t in p.items()}
    xi = _Round.apply(xr, False, rounding)  # (grad_x: rounded once, after the sum over every consumer of x)
    with _straight_through_rounding():
        out = REF.staged_reference(xi, q["conv_weights"], q["attn_l"], q["attn_r"], rel_ptrs, row, col, num_nodes, slope,
                                   q.get("loop_weight"), q.get("h_bias"), num_dst, rounding)
    leaves = [xr] + [q[n] for n in PARAMS if n in q]
    grads = iter(torch.autograd.grad(out, leaves, gradout))
    gx = next(grads)
    return [out.detach(), gx] + [next(grads) if n in q else None for n in PARAMS]


def oracle(x, p, rel_ptrs, row, col, num_nodes, gradout, slope=0.2, num_dst=None):
    """The same list from oracle/layers.py::rgat_layer in the dtype of ``x`` (no rounding; the first num_dst rows are the output)."""
    from oracle import layers as OL
    xr = x.detach().clone().requires_grad_(True)
    q = {n: t.detach().clone().requires_grad_(True) for n, t in p.items()}
    out = OL.rgat_layer(xr, q["conv_weights"], q["attn_l"], q["attn_r"], rel_ptrs, row, col, num_nodes, slope, q.get("loop_weight"),
                        q.get("h_bias"))
    out = out[:num_nodes if num_dst is None else num_dst]
    leaves = [xr] + [q[n] for n in PARAMS if n in q]
    grads = iter(torch.autograd.grad(out, leaves, gradout))
    gx = next(grads)
    return [out.detach(), gx] + [next(grads) if n in q else None for n in PARAMS]


def oracle_and_emulation(case, g, layer, xb, gob, rounding=True, dtype=torch.float64):
    """(oracle list, emulation list), NAMES in order, both from the layer's fp32 parameters (taken exactly), the bf16 input ``xb`` and
    the bf16 output gradient ``gob`` [nd, X], evaluated on the CPU in ``dtype``."""
    s = g.get_separate_coo_original()
    rp, row, col = s["rel_ptrs"].cpu(), s["row_indices"].cpu(), s["col_indices"].cpu()
    p = {n: t.detach().cpu().to(dtype) for n, t in layer.named_parameters()}
    x, go = xb.detach().cpu().to(dtype), gob.detach().cpu().to(dtype)
    N = g.get_num_nodes()
    return (oracle(x, p, rp, row, col, N, go, 0.2, case["nd"]),
            staged_emulation(x, p, rp, row, col, N, go, 0.2, case["nd"], rounding))


def rel_l2(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).norm() / ref.norm().clamp_min(1e-300))


# ---- the cases of the GPU value test: the smallest shapes at which the kernels can still go wrong ----------------------------------
SHAPES = [(4, 16, 4), (2, 16, 8), (2, 32, 4), (1, 32, 3), (1, 64, 4)]  # (H, D, R): el from the gathered row (D = 16) and el gathered
CASES = []
for _H, _D, _R in SHAPES:
    for _mf in (False, True):  # default flags and multiply_among_weights_first_flag
        CASES.append(REF._case(f"shape_H{_H}_D{_D}_R{_R}_{'folded' if _mf else 'default'}", ("random", 710 + _R, 400, _R, 9000), _H, 64,
                               _H * _D, mulfirst=_mf, seed=_H + _D))
for _H, _D in [(4, 16), (2, 32)]:
    for _sl, _b in [(True, False), (False, True), (False, False)]:
        CASES.append(REF._case(f"H{_H}_D{_D}_loop{int(_sl)}_bias{int(_b)}", ("random", 720, 400, 4, 9000), _H, 64, _H * _D, self_loop=_sl,
                               bias=_b))
CASES.append(REF._case("input_width_32", ("random", 734, 400, 4, 9000), 2, 32, 64))
CASES.append(REF._case("head_padded_from_8", ("random", 731, 400, 4, 9000), 2, 64, 16))
CASES.append(REF._case("block_num_dst", ("block", 5, 900, 4, 7000, 200), 4, 64, 64, nd=200))
CASES.append(REF._case("ladder_el_from_row", ("ladder", 5, 3), 4, 64, 64))   # hubs (runs of 257 / 513), long segments, split destinations
CASES.append(REF._case("ladder_el_gathered", ("ladder", 5, 3), 2, 64, 64))
CASE_NAMES = [c["name"] for c in CASES]


def build_case(case, bf16_training=True):
    """(graph, layer, x, gradout): on the CPU; x [N,K] and gradout [nd,X] are bf16.  The layer of REF.build_case with the keyword."""
    from het_amd.layers import HET_RGATLayer
    g = REF.build_graph(case["graph"])
    torch.manual_seed(case["seed"])
    layer = HET_RGATLayer(case["K"], case["X"], g.get_num_rels(), case["H"], bias=case["bias"], self_loop=case["self_loop"],
                          multiply_among_weights_first_flag=case["mulfirst"], dropout=0.0, bf16_training=bf16_training)
    if case["bias"]:
        with torch.no_grad():
            layer.h_bias.uniform_(-0.1, 0.1)
    N = g.get_num_nodes()
    x = (torch.randn(N, case["K"]) * 0.5).to(BF16)
    go = torch.randn(N if case["nd"] is None else case["nd"], case["X"]).to(BF16)
    return g, layer, x, go


# ---- the row-wise criterion of the GPU value test -------------------------------------------------------------------------------------
# d[v] = ||a[v] - ref[v]|| / ||ref[v]|| per output row; the layer passes when max_v d_hip[v] <= ROW_FACTOR max_v d_ref[v], d_ref from
# the staged emulation in the same run (2: the project's factor over the emulation, as for the whole-tensor distances).  Measured on
# the CPU over the 21 cases (tests/test_bf16_rows_ref.py::test_rowwise_emulation_maxima prints them): max_v d_ref 2.7e-3 .. 4.3e-3 for
# out; for grad_x 2.2e-3 .. 2.6e-3 with the self-loop term, 7.3e-3 .. 1.5e-2 without it and 1.9e-2 for block_num_dst (sources beyond nd:
# rows of a few small terms).  ROW_CAP: no case may have an emulation row looser than this, or the criterion could hide a wrong row
# behind it -- a case that exceeds it gets another input, not another cap.
ROW_FACTOR = 2.0
ROW_CAP = 2.5e-2


def row_rel(a, ref):
    """(d [rows with a non-zero reference row], mask of those rows): the relative L2 distance of every row of ``a`` to ``ref``."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    n = ref.norm(dim=1)
    nz = n > 0
    return (a - ref).norm(dim=1)[nz] / n[nz], nz


def check_rowwise(name, a, ref, emu):
    """max_v d_hip[v] <= ROW_FACTOR max_v d_ref[v]; a row whose reference is exactly zero (no term reaches it) must be exactly zero.
    Returns (max d_ref, max d_hip)."""
    d_hip, nz = row_rel(a, ref)
    d_ref, _ = row_rel(emu, ref)
    zero = a.detach().double().cpu()[~nz]
    assert float(zero.abs().max() if zero.numel() else 0.0) == 0.0, f"{name}: a row with a zero reference is not zero"
    m_ref, m_hip = float(d_ref.max()), float(d_hip.max())
    print(f"{name}: max_v d_ref {m_ref:.3e} max_v d_hip {m_hip:.3e}")
    assert m_hip <= ROW_FACTOR * m_ref, f"{name}: row {int(torch.nonzero(nz).flatten()[int(d_hip.argmax())])} is {m_hip:.3e} from the oracle, " \
                                        f"the emulation's worst row {m_ref:.3e}"
    return m_ref, m_hip
