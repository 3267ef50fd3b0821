"""References of tests/test_gpu_hgt_bf16.py that need no GPU: the explicit fp64 backward of the attention rows (formulas of
csrc/hgt_compact.hip's header comment), the staged fp64 emulation of the HGT layer's bf16 rounding points, and the bound for a
bf16 row tensor that is rounded once.  tests/test_hgt_bf16_abi.py validates the first two against the oracle on the CPU."""
import torch


def check_bf16(name, a, ref):
    """A bf16 result rounded once from an fp32 value against its fp64 reference: elementwise 2^-8 |ref| + 1e-5 max|ref| (twice the
    half-ulp of bf16) and relative L2 <= 3e-3 -- the bound tests/test_gpu_rgcn_bf16.py::_check_bf16 derives for that situation."""
    assert a.dtype == torch.bfloat16, f"{name}: {a.dtype}"
    a, ref = a.detach().double().to(ref.device), ref.detach().double()
    d = (a - ref).abs()
    rel_l2 = float((a - ref).norm() / ref.norm().clamp_min(1e-300))
    bound = 2.0 ** -8 * ref.abs() + 1e-5 * float(ref.abs().max())
    worst = float((d - bound).max())
    print(f"{name}: rel L2 {rel_l2:.2e}, max excess over the elementwise bound {worst:.2e}")
    assert rel_l2 <= 3e-3, f"{name}: relative L2 error {rel_l2:.2e}"
    assert worst <= 0, f"{name}: {int((d > bound).sum())} elements outside 2^-8 |ref| + 1e-5 max|ref|"


def attention_rows_backward(kv, q, gradout, out, srow, col):
    """grad_kv_c [S_row,2,H,D] and grad_q [N,H,D] in the dtype of the inputs (fp64), evaluated explicitly from the formulas in the
    header comment of csrc/hgt_compact.hip, with <gradout, out> taken from the GIVEN ``out`` (the kernels read the stored one):
      a_e = exp(s_e) / SUM exp(s);  ga_e = <gradout[v], m[srow_e]>;  gs_e = a_e (ga_e - <gradout, out>[v])
      grad_q[v] = SUM gs_e k'[srow_e];  grad_k'[u] = SUM gs_e q[dst_e];  grad_m[u] = SUM a_e gradout[dst_e]"""
    k, m = kv[:, 0], kv[:, 1]
    N, H, _ = q.shape
    w = torch.exp((k[srow] * q[col]).sum(-1))
    den = torch.zeros(N, H, dtype=q.dtype, device=q.device).index_add(0, col, w)
    a = w / den[col]
    ga = (gradout[col] * m[srow]).sum(-1)
    gs = a * (ga - (gradout * out).sum(-1)[col])
    gq = torch.zeros_like(q).index_add(0, col, gs.unsqueeze(-1) * k[srow])
    gk = torch.zeros_like(k).index_add(0, srow, gs.unsqueeze(-1) * q[col])
    gm = torch.zeros_like(m).index_add(0, srow, a.unsqueeze(-1) * gradout[col])
    return torch.stack([gk, gm], 1), gq


def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


class _Round(torch.autograd.Function):
    """Rounds the value to bf16 on the way forward and / or the gradient on the way back (straight-through otherwise)."""

    @staticmethod
    def forward(ctx, x, fwd, bwd):
        ctx.bwd = bwd
        return bf16_round(x) if fwd else x.clone()

    @staticmethod
    def backward(ctx, g):
        return (bf16_round(g) if ctx.bwd else g), None, None


def staged_emulation(h, offs, rel_ptrs, row, col, num_nodes, src_type, p, num_heads, fused_attn, rounding):
    """The fused HGT layer as a torch composition in the dtype of ``h`` (fp64) that rounds to bf16 exactly where the layer's bf16
    contract says (het_amd/layers.py::HET_HGTLayerHetero): kv_c and q at their products' stores, new_h and its gradient, the
    layer output, and h.grad once after all terms are summed.  ``rounding`` False: no rounding anywhere (then it is
    oracle/layers.py::hgt_layer, which test_staged_emulation_without_rounding_is_the_oracle asserts).  p: the eight parameters."""
    from het_amd.backend.hgt_fused_layer import fold_source_weights
    from oracle import ops as O
    rnd = lambda x, fwd=True, bwd=False: _Round.apply(x, fwd and rounding, bwd and rounding)
    T, R, H = offs.numel() - 1, rel_ptrs.numel() - 1, num_heads
    X = p["k_linears"].shape[3]
    h = rnd(h, False, True)  # (h.grad: the sum of all its consumers' terms, rounded once)

    def typed_linear(x, W):
        return torch.cat([x[int(offs[t]):int(offs[t + 1])] @ W[t, 0] for t in range(T)])

    w_kv = fold_source_weights(p["k_linears"], p["v_linears"], p["relation_att"], p["relation_msg"], p["relation_pri"], src_type, H,
                               fused_attn)  # [R,1,in,2X]: its torch branch (fp64 CPU / GPU tensors are not the HIP kernel's)
    rows, srow, base = [], torch.empty_like(row), 0
    for r in range(R):  # the distinct (relation, source) rows, relation by relation
        a, b = int(rel_ptrs[r]), int(rel_ptrs[r + 1])
        nodes, inv = torch.unique(row[a:b], return_inverse=True)
        rows.append(h[nodes] @ w_kv[r, 0])
        srow[a:b] = base + inv
        base += nodes.numel()
    kv_c = rnd(torch.cat(rows))
    q = rnd(typed_linear(h, p["q_linears"]))
    _, new_h = O.hgt_attention_rows(kv_c.view(-1, 2, H, X // H), q.view(-1, H, X // H), srow, col, num_nodes)
    new_h = rnd(new_h.reshape(num_nodes, X), True, True)
    return rnd(typed_linear(new_h, torch.sigmoid(p["skip"]) * p["a_linears"]))


PARAMS = ["k_linears", "q_linears", "v_linears", "a_linears", "relation_att", "relation_msg", "relation_pri", "skip"]


def oracle_and_emulation(g, layer, hb, gob, H, fused_attn, dev="cpu"):
    """(oracle, emulation): each a list [out, grad_h, grad of every parameter in PARAMS order], fp64, on the bf16-rounded ``hb`` /
    ``gob`` with the layer's fp32 parameters taken exactly."""
    from oracle import layers as OL
    s = g.get_separate_coo_original()
    offs = g.get_original_node_type_offsets().cpu()
    rp, row, col = s["rel_ptrs"].to(dev), s["row_indices"].to(dev), s["col_indices"].to(dev)
    st = g.get_rel_node_types()[0].to(dev)
    N = g.get_num_nodes()
    res = []
    for emu in (False, True):
        p = {n: getattr(layer, n).detach().double().to(dev).requires_grad_(True) for n in PARAMS}
        h64 = hb.detach().double().to(dev).requires_grad_(True)
        if emu:
            out = staged_emulation(h64, offs, rp.cpu(), row, col, N, st, p, H, fused_attn, True)
        else:
            out = OL.hgt_layer(h64, offs, rp, row, col, N, *(p[n] for n in PARAMS), H, fused_attn=fused_attn)
        grads = torch.autograd.grad(out, [h64] + [p[n] for n in PARAMS], gob.detach().double().to(dev))
        res.append([out.detach()] + list(grads))
    return res
