"""References of tests/test_gpu_hgt_use_norm.py that need no GPU: the fp64 oracle of the HGT layer with use_norm (oracle/layers.py's
hgt_layer followed by the fp64 typed LayerNorm with the layer's parameters) and the staged emulation of its bf16 contract --
tests/_hgt_bf16_ref.py::staged_emulation plus the two roundings the norm adds: grad_y (the gradient the norm's backward stores)
and out (after the fp64 norm of the bf16 y)."""
import torch

from tests._hgt_bf16_ref import PARAMS, _Round, staged_emulation
from tests._typed_layer_norm_ref import typed_layer_norm_ref

NORM_PARAMS = PARAMS + ["norm_weight", "norm_bias"]


def _params(layer, dev="cpu"):
    return {n: getattr(layer, n).detach().double().to(dev).requires_grad_(True) for n in NORM_PARAMS}


def oracle(g, layer, h, go, H, fused_attn):
    """[out, grad_h, grad of every parameter in NORM_PARAMS order] in fp64 on the CPU for the layer's fp32 parameters taken exactly."""
    from oracle import layers as OL
    s = g.get_separate_coo_original()
    offs = g.get_original_node_type_offsets().cpu()
    N = g.get_num_nodes()
    p = _params(layer)
    h64 = h.detach().double().cpu().requires_grad_(True)
    y = OL.hgt_layer(h64, offs, s["rel_ptrs"].cpu(), s["row_indices"].cpu(), s["col_indices"].cpu(), N, *(p[n] for n in PARAMS), H,
                     fused_attn=fused_attn)
    out, _, _ = typed_layer_norm_ref(y, offs, p["norm_weight"], p["norm_bias"], layer.norm_eps)
    grads = torch.autograd.grad(out, [h64] + [p[n] for n in NORM_PARAMS], go.detach().double().cpu())
    return [out.detach()] + list(grads)


def emulation(g, layer, hb, gob, H, fused_attn):
    """The same list from the staged emulation with rounding at every point of the bf16 contract (class docstring of
    het_amd/layers.py::HET_HGTLayerHetero), the norm's two included."""
    s = g.get_separate_coo_original()
    offs = g.get_original_node_type_offsets().cpu()
    N = g.get_num_nodes()
    p = _params(layer)
    h64 = hb.detach().double().cpu().requires_grad_(True)
    y = staged_emulation(h64, offs, s["rel_ptrs"].cpu(), s["row_indices"].cpu(), s["col_indices"].cpu(), N,
                         g.get_rel_node_types()[0].cpu(), {n: p[n] for n in PARAMS}, H, fused_attn, True)  # (y: rounded at its store)
    y = _Round.apply(y, False, True)  # grad_y: rounded once where the norm's backward stores it
    out, _, _ = typed_layer_norm_ref(y, offs, p["norm_weight"], p["norm_bias"], layer.norm_eps)
    out = _Round.apply(out, True, False)  # out: rounded once at the norm's store
    grads = torch.autograd.grad(out, [h64] + [p[n] for n in NORM_PARAMS], gob.detach().double().cpu())
    return [out.detach()] + list(grads)
