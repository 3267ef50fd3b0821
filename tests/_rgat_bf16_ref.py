"""References of tests/test_gpu_rgat_bf16.py that need no GPU: the staged emulation of the RGAT layer's bf16 evaluation contract
(het_amd/backend/rgat_fused_layer.py: _forward_only_bf16), the cases the GPU value test runs, and the measurement of the absolute
term of its bound.  tests/test_rgat_bf16_ref.py validates the emulation against the oracle on the CPU."""
import torch

from tests.util import ladder_graph, random_graph

BF16 = torch.bfloat16


def bf16_round(t):
    return t.to(BF16).to(t.dtype)


def staged_reference(x, W, attn_l, attn_r, rel_ptrs, row, col, num_nodes, slope=0.2, loop_weight=None, h_bias=None, num_dst=None,
                     rounding=True):
    """The layer in the dtype of ``x`` (fp64, or fp32 for the measurement below), rounding to bf16 exactly where the contract says:
      feat_c = round(x[u] . W[r])           on the distinct (relation, source) rows, at the projection's store
      el_c   = <feat_c, attn_l[r]>           from the ROUNDED row, not rounded itself
      er_c   = <x[v], W[r] . attn_r[r]>      the folded weight, not rounded
      h      = round(x[:nd] . loop_w + bias) the bias added before the rounding
      out[v] = round(h[v] + SUM_e softmax_v(leaky(el + er))_e feat_c[srow_e])   for destinations with in-edges; h[v] otherwise
    ``rounding`` False: no rounding anywhere -- then it is oracle/layers.py::rgat_layer (first num_dst rows)."""
    rnd = bf16_round if rounding else (lambda t: t)
    R, H, K, D = W.shape
    X = H * D
    nd = num_nodes if num_dst is None else num_dst
    feat, el, er = [], [], []
    for r in range(R):
        a, b = int(rel_ptrs[r]), int(rel_ptrs[r + 1])
        nodes, inv = torch.unique(row[a:b], return_inverse=True)
        fc = rnd(x[nodes] @ W[r].permute(1, 0, 2).reshape(K, X)).view(-1, H, D)
        feat.append(fc[inv])
        el.append((fc * attn_l[r]).sum(-1)[inv])
        wa = (W[r] @ attn_r[r].unsqueeze(-1)).squeeze(-1)  # [H,K]
        er.append(x[col[a:b]] @ wa.t())
    feat, z = torch.cat(feat), torch.cat(el) + torch.cat(er)
    s = torch.where(z > 0, z, z * slope)
    m = torch.full((num_nodes, H), -float("inf"), dtype=x.dtype).scatter_reduce(0, col.unsqueeze(-1).expand(-1, H), s, "amax")
    w = torch.exp(s - m[col])
    den = torch.zeros(num_nodes, H, dtype=x.dtype).index_add(0, col, w)
    agg = torch.zeros(num_nodes, H, D, dtype=x.dtype).index_add(0, col, (w / den[col]).unsqueeze(-1) * feat).view(num_nodes, X)[:nd]
    h = torch.zeros(nd, X, dtype=x.dtype)
    if loop_weight is not None:
        h = h + x[:nd] @ loop_weight
    if h_bias is not None:
        h = h + h_bias
    return rnd(rnd(h) + agg)  # (rows without in-edges: agg == 0 and round(round(h)) == round(h) -- untouched)


# ---- the cases of the GPU value test ------------------------------------------------------------------------------------
def _case(name, graph, H, K, X, mulfirst=False, self_loop=True, bias=True, nd=None, seed=0):
    return dict(name=name, graph=graph, H=H, K=K, X=X, mulfirst=mulfirst, self_loop=self_loop, bias=bias, nd=nd, seed=seed)


CASES = []
for _H, _D, _R in [(4, 16, 4), (2, 16, 8), (2, 32, 4), (1, 32, 3), (1, 64, 4), (8, 16, 5), (4, 16, 9)]:
    for _mf in (False, True):  # default and folded flags
        CASES.append(_case(f"shape_H{_H}_D{_D}_R{_R}_{'folded' if _mf else 'default'}", ("random", 710 + _R, 400, _R, 9000), _H, 64, _H * _D,
                           mulfirst=_mf, seed=_H + _D))
for _sl, _b in [(True, False), (False, True), (False, False)]:
    CASES.append(_case(f"loop{int(_sl)}_bias{int(_b)}", ("random", 720, 350, 4, 6000), 4, 64, 64, self_loop=_sl, bias=_b))
    CASES.append(_case(f"loop{int(_sl)}_bias{int(_b)}_gathered_el", ("random", 720, 350, 4, 6000), 2, 64, 64, self_loop=_sl, bias=_b))
CASES.append(_case("block_num_dst", ("block", 5, 900, 4, 7000, 200), 4, 64, 64, nd=200))
CASES.append(_case("block_num_dst_no_loop", ("block", 5, 900, 4, 7000, 200), 4, 64, 64, nd=200, self_loop=False))
CASES.append(_case("hub_el_from_row", ("ladder", 5, 3), 4, 64, 64, mulfirst=True))
CASES.append(_case("hub_el_gathered", ("ladder", 5, 3), 2, 64, 64, mulfirst=True))
CASES.append(_case("hub_nine_relations", ("ladder", 9, 3), 4, 64, 64))
CASES.append(_case("head_padded_from_8", ("random", 731, 400, 4, 9000), 2, 64, 16))
CASES.append(_case("input_width_100", ("random", 732, 400, 5, 9000), 4, 100, 64))
CASES.append(_case("input_width_100_head_8", ("random", 733, 400, 3, 9000), 2, 100, 16))
CASES.append(_case("input_width_32", ("random", 734, 400, 4, 9000), 2, 32, 64))
CASE_NAMES = [c["name"] for c in CASES]


def build_graph(spec):
    from het_amd.graph import HetGraph
    from het_amd.synth import IntegratedCOO
    if spec[0] == "random":
        _, seed, n, r, e = spec
        return random_graph(seed=seed, n=n, r=r, e=e, shuffle=False, empty_rel=r > 2)
    if spec[0] == "ladder":
        return ladder_graph(R=spec[1], seed=spec[2], shuffle=False)
    _, seed, N, R, E, nd = spec  # a block: every edge points at one of the first nd nodes
    gen = torch.Generator().manual_seed(seed)
    rel = torch.sort(torch.randint(0, R, (E,), generator=gen)).values
    return HetGraph.from_integrated_coo(IntegratedCOO(N, R, torch.tensor([0, N]), torch.randint(0, N, (E,), generator=gen),
                                                      torch.randint(0, nd, (E,), generator=gen), rel, torch.arange(E)))


def build_case(case):
    """(graph, layer, x): on the CPU; x is bf16."""
    from het_amd.layers import HET_RGATLayer
    g = build_graph(case["graph"])
    torch.manual_seed(case["seed"])
    layer = HET_RGATLayer(case["K"], case["X"], g.get_num_rels(), case["H"], bias=case["bias"], self_loop=case["self_loop"],
                          multiply_among_weights_first_flag=case["mulfirst"], dropout=0.0)
    if case["bias"]:
        with torch.no_grad():
            layer.h_bias.uniform_(-0.1, 0.1)
    x = (torch.randn(g.get_num_nodes(), case["K"]) * 0.5).to(BF16)
    return g, layer, x


def reference_of(case, g, layer, x, dtype=torch.float64, rounding=True):
    """The staged reference of a case from the layer's fp32 parameters (taken exactly) and the bf16 input, evaluated in ``dtype``."""
    s = g.get_separate_coo_original()
    p = {n: t.detach().cpu().to(dtype) for n, t in layer.named_parameters()}
    return staged_reference(x.detach().cpu().to(dtype), p["conv_weights"], p["attn_l"], p["attn_r"], s["rel_ptrs"].cpu(),
                            s["row_indices"].cpu(), s["col_indices"].cpu(), g.get_num_nodes(), 0.2, p.get("loop_weight"),
                            p.get("h_bias"), case["nd"], rounding)


REL = 2.0 ** -8  # twice the half-ulp of bf16: the final rounding, and one more for a value that sits next to a rounding boundary


def smallest_abs_term(out, ref):
    """The smallest a for which every element of ``out`` satisfies |out - ref| <= 2^-8 |ref| + a max|ref|."""
    out, ref = out.double(), ref.double()
    return max(0.0, float(((out - ref).abs() - REL * ref.abs()).max() / ref.abs().max()))


def measure_abs_term():
    """max over CASES of the smallest a for which the fp32 evaluation of the staged reference passes against the fp64 one: what
    the order of the fp32 sums alone does to a result with bf16 roundings inside it (an intermediate that lands on the other side
    of a rounding boundary moves a feat_c or h element by a whole bf16 unit).  Returns (worst, per-case list)."""
    per = []
    for case in CASES:
        g, layer, x = build_case(case)
        per.append((case["name"], smallest_abs_term(reference_of(case, g, layer, x, torch.float32), reference_of(case, g, layer, x))))
    return max(v for _, v in per), per
