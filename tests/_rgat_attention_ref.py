"""References of tests/test_gpu_rgat_attention.py that need no GPU: the attention weights of the RGAT layer in the arithmetic of
oracle/layers.py::rgat_layer, returned in edge-id order; the staged variant for bf16 activations (the roundings of
tests/_rgat_bf16_ref.py); the cases of the GPU value tests; and the measurement their bounds come from."""
import functools

import torch

from tests._rgat_bf16_ref import BF16, bf16_round
from tests.util import ladder_graph, permute_eids, random_graph

FLOOR = 1e-4  # deviations are taken relative to max(a, FLOOR): a weight below 1e-4 decides no plot, pruning or explanation, and the
#               relative error of exp(s - lse) grows with |s - lse| (an absolute error of the score), so the far tail has no fixed one


def _softmax_by_destination(z, col, num_nodes, slope):
    """a [E,H] by position: exponentials relative to the destination's maximum (oracle: exp(leaky(z)) / SUM; the same number
    wherever that is finite)."""
    H = z.shape[1]
    s = torch.where(z > 0, z, z * slope)
    m = torch.full((num_nodes, H), -float("inf"), dtype=z.dtype).scatter_reduce(0, col.unsqueeze(-1).expand(-1, H), s, "amax")
    w = torch.exp(s - m[col])
    den = torch.zeros(num_nodes, H, dtype=z.dtype).index_add(0, col, w)
    return w / den[col]


def attention_reference(x, W, attn_l, attn_r, rel_ptrs, row, col, eids, num_nodes, slope=0.2):
    """(a [E,H] with row i = edge id i, feat [E,H,D] by position) in the dtype of ``x``: rgat_layer's per-relation projections of both
    ends of every edge and the dots with attn_l / attn_r."""
    R, H, K, D = W.shape
    fl, zl = [], []
    for r in range(R):
        a, b = int(rel_ptrs[r]), int(rel_ptrs[r + 1])
        Wr = W[r].permute(1, 0, 2).reshape(K, H * D)
        fs = (x[row[a:b]] @ Wr).view(-1, H, D)
        fd = (x[col[a:b]] @ Wr).view(-1, H, D)
        fl.append(fs)
        zl.append((fs * attn_l[r]).sum(-1) + (fd * attn_r[r]).sum(-1))
    a_pos = _softmax_by_destination(torch.cat(zl), col, num_nodes, slope)
    a = torch.empty_like(a_pos)
    a[eids] = a_pos
    return a, torch.cat(fl)


def staged_attention_reference(x, W, attn_l, attn_r, rel_ptrs, row, col, eids, num_nodes, slope=0.2):
    """a [E,H] in edge-id order under the bf16 contract (tests/_rgat_bf16_ref.py::staged_reference): el from the ROUNDED feat_c row of
    the distinct (relation, source) rows, er from the widened x and the folded weight, nothing else rounded."""
    R, H, K, D = W.shape
    zl = []
    for r in range(R):
        a, b = int(rel_ptrs[r]), int(rel_ptrs[r + 1])
        nodes, inv = torch.unique(row[a:b], return_inverse=True)
        fc = bf16_round(x[nodes] @ W[r].permute(1, 0, 2).reshape(K, H * D)).view(-1, H, D)
        wa = (W[r] @ attn_r[r].unsqueeze(-1)).squeeze(-1)  # [H,K]
        zl.append((fc * attn_l[r]).sum(-1)[inv] + x[col[a:b]] @ wa.t())
    a_pos = _softmax_by_destination(torch.cat(zl), col, num_nodes, slope)
    a = torch.empty_like(a_pos)
    a[eids] = a_pos
    return a


# ---- the cases --------------------------------------------------------------------------------------------------------------------
SHAPES = [(4, 16), (2, 32), (1, 64), (8, 16)]
RELS = [3, 5, 9]
VALUE_CASES = [(kind, R, H, D) for kind in ("random", "ladder") for R in RELS for (H, D) in SHAPES]
LARGE_SCALE = 400.0  # attn_l and attn_r times this: max |el + er| is above 100 on the large-score case (asserted by its test)
BF16_CASES = [("random", 5, 4, 16), ("random", 5, 2, 32), ("ladder", 5, 4, 16), ("ladder", 5, 2, 32)]  # el from the row / gathered


def build_graph(kind, R, shuffle=False):
    """random_graph: 257 nodes, 3001 edges, an empty relation, nodes without in-edges; ladder_graph: in-degrees on both sides of the
    32 / 64 pack and the 256 split thresholds.  ``shuffle``: the eids are a random permutation of the positions."""
    g = random_graph(seed=900 + R, r=R, shuffle=False) if kind == "random" else ladder_graph(R=R, seed=3, shuffle=False)
    if shuffle:
        permute_eids(g, 1900 + R)
    return g


def build_case(kind, R, H, D, shuffle=False, scale=1.0, bf16=False, K=64):
    """(graph, layer, x) on the CPU."""
    from het_amd.layers import HET_RGATLayer
    g = build_graph(kind, R, shuffle)
    torch.manual_seed(H + D + R)
    layer = HET_RGATLayer(K, H * D, g.get_num_rels(), H, bias=True, self_loop=True, dropout=0.0)
    with torch.no_grad():
        layer.h_bias.uniform_(-0.1, 0.1)
        layer.attn_l.mul_(scale)
        layer.attn_r.mul_(scale)
    x = torch.randn(g.get_num_nodes(), K) * 0.5
    return g, layer, (x.to(BF16) if bf16 else x)


def reference_of(g, layer, x, dtype=torch.float64, staged=False):
    """The reference of a case from the layer's fp32 parameters and its input (both taken exactly), evaluated in ``dtype``:
    (a, feat) -- feat None for the staged one."""
    s = g.get_separate_coo_original()
    p = {n: t.detach().cpu().to(dtype) for n, t in layer.named_parameters()}
    args = (x.detach().cpu().to(dtype), p["conv_weights"], p["attn_l"], p["attn_r"], s["rel_ptrs"].cpu(), s["row_indices"].cpu(),
            s["col_indices"].cpu(), s["eids"].cpu(), g.get_num_nodes(), 0.2)
    if staged:
        return staged_attention_reference(*args), None
    return attention_reference(*args)


def max_abs_score(g, layer, x):
    """max |el + er| over the (edge, head) pairs, in fp64."""
    s = g.get_separate_coo_original()
    W = layer.conv_weights.detach().cpu().double()
    rel = torch.repeat_interleave(torch.arange(W.shape[0]), s["rel_ptrs"][1:] - s["rel_ptrs"][:-1])
    wl = torch.einsum("rhkd,rhd->rhk", W, layer.attn_l.detach().cpu().double())
    wr = torch.einsum("rhkd,rhd->rhk", W, layer.attn_r.detach().cpu().double())
    x = x.detach().cpu().double()
    z = torch.einsum("ek,ehk->eh", x[s["row_indices"]], wl[rel]) + torch.einsum("ek,ehk->eh", x[s["col_indices"]], wr[rel])
    return float(z.abs().max())


def deviation(a, ref):
    """max |a - ref| / max(ref, FLOOR)."""
    a, ref = a.detach().cpu().double(), ref.double()
    return float(((a - ref).abs() / ref.clamp_min(FLOOR)).max()) if ref.numel() else 0.0


@functools.lru_cache(maxsize=None)
def measure(family):
    """The largest deviation of the reference evaluated in fp32 on the CPU from itself in fp64 over the cases of a family: what
    fp32 rounding and one summation order do to the weights.  The GPU is allowed 4 x this (its order is a third one)."""
    if family == "fp32":
        cases = [dict(kind=k, R=R, H=H, D=D) for (k, R, H, D) in VALUE_CASES]
    elif family == "large":
        cases = [dict(kind="ladder", R=5, H=4, D=16, scale=LARGE_SCALE), dict(kind="random", R=5, H=2, D=32, scale=LARGE_SCALE)]
    else:
        cases = [dict(kind=k, R=R, H=H, D=D, bf16=True) for (k, R, H, D) in BF16_CASES]
    worst = 0.0
    for c in cases:
        g, layer, x = build_case(**c)
        staged = family == "bf16"
        worst = max(worst, deviation(reference_of(g, layer, x, torch.float32, staged)[0], reference_of(g, layer, x, torch.float64, staged)[0]))
    return worst
