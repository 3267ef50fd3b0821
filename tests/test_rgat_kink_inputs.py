"""The conditions of the exact inputs the kink tests run on (tests/util.py: exact_rgat_case, exact_gat_case; the GPU tests
are tests/test_gpu_rgat_kink.py), on the CPU.  They are conditions of the generators, not measurements: if one fails, the grid
changes, not the bound.  And the reason for the inputs: a leaky-ReLU derivative that takes the wrong branch AT z == 0 (z >= 0
where the reference's gradLeaky and the oracle say z > 0) is rejected by tests/util.py::assert_close on all four gradients that
pass through the attention, while the forward output does not move."""
import functools

import pytest
import torch

from oracle import layers as OL
from tests.util import (GAT_Z_CLASSES, LADDER, LADDER_SPLITS, TINY, assert_close, assert_ties_on_hub_edges, exact_gat_case_of_kind,
                        exact_rgat_case, gat_rows_of_kind, gat_z_class, ladder_graph, rgat_case_preactivations, rgat_case_tie_stats)

H, D = 4, 16


@functools.lru_cache(maxsize=None)
def _graph(R):
    return ladder_graph(R=R)


def _bf16_exact(t):
    return torch.equal(t.to(torch.bfloat16).float(), t)


@pytest.mark.parametrize("R", [5, 9])
@pytest.mark.parametrize("K", [64, 32])
def test_layer_case_is_exact_and_sits_on_the_kink(R, K):
    g = _graph(R)
    s = g.get_separate_coo_original()
    N = g.get_num_nodes()
    c = exact_rgat_case(g, H, K, D, seed=3)
    z64 = rgat_case_preactivations(c, s)
    # the same z, bit for bit, in fp32 in both associations and with the projected rows rounded to bf16
    for kw in ({}, {"folded": True}, {"bf16_feat": True}):
        z32 = rgat_case_preactivations(c, s, dtype=torch.float32, **kw)
        assert z32.dtype == torch.float32 and torch.equal(z32.double(), z64), kw
    assert torch.equal(rgat_case_preactivations(c, s, folded=True), z64)
    feat = torch.einsum("nk,rhkd->rnhd", c["x"], c["W"])
    assert _bf16_exact(c["x"]) and _bf16_exact(feat) and _bf16_exact(c["go"])
    # ties: at least 2 % of the pairs, in every relation that has edges, on hubs and on a destination of one in-edge
    tie = z64 == 0
    assert float(tie.float().mean()) >= 0.02, float(tie.float().mean())
    rp = s["rel_ptrs"].tolist()
    for r, (a, b) in enumerate(zip(rp[:-1], rp[1:])):
        assert b == a or bool(tie[a:b].any()), f"relation {r} has no tie"
    st = rgat_case_tie_stats(c, s, N)
    assert st["hub"] >= 100 and st["deg1"] >= 1, st
    assert_ties_on_hub_edges(c, s, N, hub=100)
    assert float((z64 > 0).float().mean()) >= 0.25 and float((z64 < 0).float().mean()) >= 0.25
    assert float(z64[~tie].abs().min()) >= 1 / 16
    p = [c[n].double() for n in ("x", "W", "attn_l", "attn_r")]
    ref = OL.rgat_layer(*p, s["rel_ptrs"], s["row_indices"], s["col_indices"], N, 0.2, c["loop_weight"].double(), c["h_bias"].double())
    assert bool(torch.isfinite(ref).all())


def _layer_with_tie_rule(c, s, N, slope, tie_is_positive):
    """oracle/layers.py::rgat_layer restated with the branch at z == 0 as a switch (False: the oracle's z > 0), and its gradients
    for the case's output gradient."""
    leaves = {n: c[n].double().requires_grad_(True) for n in ("x", "W", "attn_l", "attn_r")}
    x, W, al, ar = leaves.values()
    R = W.shape[0]
    rel = OL.rel_of_position(s["rel_ptrs"])
    feat_n = torch.einsum("nk,rhkd->rnhd", x, W)
    feat = feat_n[rel, s["row_indices"]]
    z = (feat * al[rel]).sum(-1) + (feat_n[rel, s["col_indices"]] * ar[rel]).sum(-1)
    pos = (z >= 0) if tie_is_positive else (z > 0)
    e = torch.exp(torch.where(pos, z, z * slope))
    col = s["col_indices"]
    den = torch.zeros(N, H, dtype=torch.float64).index_add(0, col, e)
    out = torch.zeros(N, H, D, dtype=torch.float64).index_add(0, col, (e / den[col]).unsqueeze(-1) * feat).view(N, H * D)
    out = out + x @ c["loop_weight"].double() + c["h_bias"].double()
    grads = torch.autograd.grad(out, list(leaves.values()), c["go"].double())
    return out.detach(), dict(zip(("grad_x", "grad_W", "grad_attn_l", "grad_attn_r"), grads))


@pytest.mark.parametrize("slope", [0.2, 0.0, 2.5])
def test_a_wrong_tie_rule_is_seen(slope):
    g = _graph(5)
    s = g.get_separate_coo_original()
    N = g.get_num_nodes()
    c = exact_rgat_case(g, H, 64, D, seed=3)
    out, grads = _layer_with_tie_rule(c, s, N, slope, False)
    # (the restatement is the oracle)
    leaves = [c[n].double().requires_grad_(True) for n in ("x", "W", "attn_l", "attn_r")]
    ref = OL.rgat_layer(*leaves, s["rel_ptrs"], s["row_indices"], s["col_indices"], N, slope, c["loop_weight"].double(), c["h_bias"].double())
    assert_close(out, ref.detach(), rtol=1e-12, atol=1e-13, what="restated oracle")
    for (n, a), b in zip(grads.items(), torch.autograd.grad(ref, leaves, c["go"].double())):
        assert_close(a, b, rtol=1e-12, atol=1e-13, what="restated oracle " + n)
    out_m, grads_m = _layer_with_tie_rule(c, s, N, slope, True)
    assert torch.equal(out_m, out)  # exp(0) on either branch: the kink does not move the forward
    for n in grads:
        with pytest.raises(AssertionError):
            assert_close(grads_m[n], grads[n], what=n)


@pytest.mark.parametrize("R", [5, 9])
@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4])
def test_op_case_has_every_class_of_z_at_every_rung(kind, R):
    g = _graph(R)
    s = g.get_separate_coo_original()
    N = g.get_num_nodes()
    srow, drow, (ns, nd) = gat_rows_of_kind(g, kind)
    col = s["col_indices"]
    feat, el, er, go = exact_gat_case_of_kind(g, kind, H, D, seed=17)  # (what tests/test_gpu_rgat_kink.py runs on)
    assert feat.shape == (ns, H, D) and el.shape == (ns, H) and er.shape == (nd, H) and go.shape == (N, H, D)
    z32 = el[srow] + er[drow]
    z64 = el.double()[srow] + er.double()[drow]
    assert z32.dtype == torch.float32 and torch.equal(z32.double(), z64)
    assert _bf16_exact(feat) and _bf16_exact(go)
    cls = gat_z_class(z64)
    assert int((cls < 0).sum()) == 0 and float(z64.abs().max()) <= 4.0
    assert float(torch.exp(torch.tensor(TINY))) == 1.0  # fp32: the stored exp of the tiny positive class is 1 unless bumped
    indeg = torch.bincount(col, minlength=N)
    rungs = torch.nonzero(indeg >= 8).flatten()
    assert rungs.numel() == sum(c >= 8 for c in LADDER) + len(LADDER_SPLITS)  # the rungs are the only such destinations
    for k, name in enumerate(GAT_Z_CLASSES):
        has = torch.zeros(N, H).index_add_(0, col, (cls == k).float()) > 0
        assert bool(has[rungs].all()), f"class {name} is missing at destinations {rungs[~has[rungs].all(1)].tolist()}"
        assert float((cls == k).float().mean()) >= 0.02, name


@pytest.mark.parametrize("K", [64, 32])
def test_bf16_training_contract_rounds_only_its_two_stores_on_the_exact_case(K):
    """On the exact case x, feat_c, the self-loop + bias rows and the output gradient are bf16 numbers already: the staged emulation of
    the bf16 training contract (tests/_rgat_bf16_train_ref.py) differs from the fp64 oracle by the roundings of the output and of
    grad_x alone -- elementwise within the bound of the bf16 ladders (tests/_bf16_rows_ref.py::check_bf16) -- and its parameter
    gradients are the oracle's.  That is what lets tests/test_gpu_rgat_kink.py hold the HIP step elementwise."""
    from tests import _bf16_rows_ref as RR
    from tests import _rgat_bf16_train_ref as TREF
    g = _graph(5)
    s = g.get_separate_coo_original()
    N = g.get_num_nodes()
    c = exact_rgat_case(g, H, K, D, seed=3)
    p = {n: c[k].double() for n, k in (("conv_weights", "W"), ("attn_l", "attn_l"), ("attn_r", "attn_r"), ("loop_weight", "loop_weight"),
                                       ("h_bias", "h_bias"))}
    h = c["x"] @ c["loop_weight"] + c["h_bias"]
    assert _bf16_exact(h)
    args = (c["x"].double(), p, s["rel_ptrs"], s["row_indices"], s["col_indices"], N, c["go"].double(), 0.2)
    ref, emu = TREF.oracle(*args), TREF.staged_emulation(*args)
    for n, r, e in zip(TREF.NAMES, ref, emu):
        if n in ("out", "grad_x"):
            assert torch.equal(e.to(torch.bfloat16).double(), e)
            RR.check_bf16(n, e.to(torch.bfloat16), r)
        else:
            assert_close(e, r, rtol=1e-12, atol=1e-13, what=n)
