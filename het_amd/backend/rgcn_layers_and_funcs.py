"""RGCN ops behind torch.autograd; mirrors
/root/reference/hrt/python/backend/rgcn_layers_and_funcs.py:481-824."""
import os

import torch as th

from ..plan import consistent as _consistent_plan

from .. import kernels as _k
from ..kernels import K

# the layer as two library calls (include/het_amd.h: het_rgcn_layer_forward / _backward); HET_RGCN_FUSED=0: the a7 / a8 pair
FUSED = os.environ.get("HET_RGCN_FUSED", "1") != "0"

__all__ = [
    "RgcnLayer1SeparateCoo", "RgcnLayerFused", "rgcn_layer1_separate_coo", "rgcn_layer_fused_applies", "RGCNNodeMeanAggregationCompactAsOfNodeSeparateCOO",
    "RgcnLayerBdd", "rgcn_layer_bdd", "rgcn_bdd_route", "rgcn_bdd_route_of", "bdd_dense_weight",
    "RGCNNodeMeanAggregationCompactAsOfNodeDirectIndexingSeparateCOO",
    "rgcn_node_mean_aggregation_compact_as_of_node_separate_coo_single_sided",
]


@_consistent_plan
class RgcnLayer1SeparateCoo(th.autograd.Function):
    # reference: rgcn_layers_and_funcs.py:481-567 (the out-CSR arguments are carried but unused there too)
    @staticmethod
    def forward(ctx, separate_coo_rel_ptrs, separate_coo_eids, separate_coo_row_indices, separate_coo_col_indices,
                outcsr_row_ptr, outcsr_col_indices, outcsr_eids, outcsr_reltypes, x, weight, norm, ret):
        ctx.save_for_backward(separate_coo_rel_ptrs, separate_coo_eids, separate_coo_row_indices,
                              separate_coo_col_indices, weight, norm, x)
        K.rgcn_layer1_separate_coo(separate_coo_rel_ptrs, separate_coo_eids, separate_coo_row_indices,
                                   separate_coo_col_indices, x, weight, norm, ret)
        return ret

    @staticmethod
    def backward(ctx, gradout):
        rel_ptrs, eids, row, col, weight, norm, x = ctx.saved_tensors
        grad_x = th.zeros_like(x, memory_format=th.contiguous_format)
        grad_weight = th.zeros_like(weight, memory_format=th.contiguous_format)
        grad_norm = th.zeros_like(norm, memory_format=th.contiguous_format)
        K.backward_rgcn_layer1_separate_coo(rel_ptrs, eids, row, col, x, th.transpose(weight, 1, 2).contiguous(), norm,
                                            grad_norm, grad_x, gradout.contiguous(), grad_weight)
        return None, None, None, None, None, None, None, None, grad_x, grad_weight, grad_norm, None


@_consistent_plan
class RgcnLayer1SeparateCooBias(th.autograd.Function):
    """RgcnLayer1SeparateCoo with the layer's bias (RGCN/RGCN.py:338-340, ``node_repr + h_bias``) inside the node: the op
    accumulates into ``ret`` (reference contract), so ``ret`` starts from the bias rows instead of zeros -- one fill instead
    of a fill and an elementwise add; the bias gradient is the column sum of gradout."""

    @staticmethod
    def forward(ctx, rel_ptrs, eids, row, col, num_nodes, x, weight, norm, bias):
        ctx.save_for_backward(rel_ptrs, eids, row, col, weight, norm, x)
        ret = bias.to(weight.dtype).expand(num_nodes, weight.size(2)).contiguous()
        K.rgcn_layer1_separate_coo(rel_ptrs, eids, row, col, x, weight, norm, ret)
        return ret

    @staticmethod
    def backward(ctx, gradout):
        rel_ptrs, eids, row, col, weight, norm, x = ctx.saved_tensors
        gradout = gradout.contiguous()
        grad_x = th.zeros_like(x, memory_format=th.contiguous_format)
        grad_weight = th.zeros_like(weight, memory_format=th.contiguous_format)
        grad_norm = th.zeros_like(norm, memory_format=th.contiguous_format)
        K.backward_rgcn_layer1_separate_coo(rel_ptrs, eids, row, col, x, th.transpose(weight, 1, 2).contiguous(), norm,
                                            grad_norm, grad_x, gradout, grad_weight)
        return None, None, None, None, None, grad_x, grad_weight, grad_norm, gradout.sum(0)


@_consistent_plan
class RgcnLayerFused(th.autograd.Function):
    """rgcn_layer1_separate_coo (+ the layer's bias, RGCN/RGCN.py:338-340) as two library calls: the sums of the scaled source
    rows per (relation, destination) are kept from the forward -- the weight gradient is formed from them (half as many rows as
    the (relation, source) sums of a8, and x is not read again) -- the output and the input gradient are written once by a pass
    over the nodes (no zero-filled buffers, no read-modify-write per relation, no transposed-weight / bias-sum torch kernels):
    ogbn-mag, feat 64: 3.0 -> 2.3 ms per step.  Same values as RgcnLayer1SeparateCooBias up to the order of the fp32 sums.
    A bf16 ``x`` takes the bf16 entries: the output and grad_x are bf16 (rounded once, when stored), the weight, norm and bias
    gradients and every sum fp32."""

    @staticmethod
    def forward(ctx, plan, x, weight, norm, bias):
        ctx.bf16 = x.dtype == th.bfloat16
        ret, ssum = (_k.rgcn_layer_forward_bf16 if ctx.bf16 else _k.rgcn_layer_forward)(plan, x, weight, norm, bias)
        ctx.plan, ctx.has_bias = plan, bias is not None
        ctx.save_for_backward(weight, norm, ssum)
        return ret

    @staticmethod
    def backward(ctx, gradout):
        weight, norm, ssum = ctx.saved_tensors
        backward = _k.rgcn_layer_backward_bf16 if ctx.bf16 else _k.rgcn_layer_backward
        grad_x, grad_w, grad_bias = backward(ctx.plan, ssum, weight.transpose(1, 2).contiguous(), norm,
                                             gradout.to(th.bfloat16 if ctx.bf16 else th.float32).contiguous(), ctx.has_bias,
                                             want_x=ctx.needs_input_grad[1])
        # (the reference's a8 takes a grad_norm buffer and leaves it as it was given: zeros)
        grad_norm = th.zeros_like(norm) if ctx.needs_input_grad[3] else None
        return None, grad_x, grad_w, grad_norm, grad_bias


def _fused_plan(graph, s, x, weight, norm, bias):
    """The plan of the two-call layer when it applies: GPU tensors of the graph's size (x float32 or bfloat16, the weight, norm and
    bias float32), shapes the node-major pass takes, groupings switched on."""
    if not (FUSED and x.is_cuda and x.dim() == 2 and weight.dim() == 3 and _k._plan.is_enabled()):
        return None
    N, E = graph.get_num_nodes(), s["eids"].numel()
    R, Kin, D = weight.shape
    if not (E > 0 and x.shape == (N, Kin) and norm.numel() == E and x.dtype in (th.float32, th.bfloat16) and
            weight.dtype == norm.dtype == th.float32 and
            (bias is None or (bias.dtype == th.float32 and bias.numel() == D)) and R == s["rel_ptrs"].numel() - 1 and
            _k.rgcn_layer_ok(R, Kin, D)):
        return None
    return _k.rgcn_layer_plan(s["rel_ptrs"], s["eids"], s["row_indices"], s["col_indices"], N)


def rgcn_layer_fused_applies(graph, x, weight, norm, bias=None) -> bool:
    """Whether rgcn_layer1_separate_coo runs these arguments as the two-call layer (for a bf16 x: the bf16 kernels)."""
    return _fused_plan(graph, graph.get_separate_coo_original(), x, weight, norm, bias) is not None


def rgcn_layer1_separate_coo(graph, x, weight, norm, bias=None):
    # reference: rgcn_layers_and_funcs.py:570-601
    s = graph.get_separate_coo_original()
    plan = _fused_plan(graph, s, x, weight, norm, bias)
    if plan is not None:
        return RgcnLayerFused.apply(plan, x.contiguous(), weight.contiguous(), norm.contiguous(),
                                    None if bias is None else bias.contiguous())
    if x.dtype == th.bfloat16 and weight.dtype == th.float32:
        # (no bf16 kernels on this path: fp32 on an upcast copy, the result rounded back -- correct, not faster)
        return rgcn_layer1_separate_coo(graph, x.float(), weight, norm, bias).to(th.bfloat16)
    if bias is not None:
        return RgcnLayer1SeparateCooBias.apply(s["rel_ptrs"], s["eids"], s["row_indices"], s["col_indices"], graph.get_num_nodes(),
                                               x.contiguous(), weight.contiguous(), norm.contiguous(), bias)
    o = graph.get_out_csr()
    ret = th.zeros((graph.get_num_nodes(), weight.size(2)), dtype=weight.dtype, device=weight.device)
    return RgcnLayer1SeparateCoo.apply(s["rel_ptrs"], s["eids"], s["row_indices"], s["col_indices"], o["row_ptrs"],
                                       o["col_indices"], o["eids"], o["rel_types"], x.contiguous(), weight.contiguous(),
                                       norm.contiguous(), ret)


# ---- block-diagonal relation weights (regularizer="bdd"): weight [R, B, K/B, D/B] ------------------------------------------
def bdd_dense_weight(weight):
    """The [R, K, D] relation weights of block-diagonal ``weight`` [R, B, si, so]: block b of relation r on the diagonal at rows
    b*si .., columns b*so .., zeros elsewhere (torch.block_diag per relation, as one differentiable expression)."""
    R, nb, si, so = weight.shape
    eye = th.eye(nb, dtype=weight.dtype, device=weight.device)
    return (weight.unsqueeze(3) * eye.view(1, nb, 1, nb, 1)).reshape(R, nb * si, nb * so)


BDD_DENSE_UP_TO_RELS = 4  # rgcn_bdd_route: relation counts measured faster on the dense two-call layer (where it applies)


def rgcn_bdd_route(*, cuda, fp32, groupings, shape_ok, compact_flag=False, env_on=True, few_rels_dense=False) -> str:
    """Which code serves a bdd layer call, from plain facts: ``"native"`` (csrc/rgcn_bdd.hip through RgcnLayerBdd) or ``"dense"``
    (the blocks expanded to [R, K, D] by bdd_dense_weight, then the layer's existing code, whatever it runs for these arguments).

    native needs ALL of: ``cuda`` and ``fp32`` -- x a float32 GPU tensor (a bf16 x keeps the dense layer's upcast behaviour) --;
    ``groupings`` -- het_amd.plan on for this thread (off inside sampling.one_shot_graphs, so sampled blocks go dense) --;
    ``shape_ok`` -- kernels.rgcn_bdd_ok(R, K, D, B) on the UNPADDED widths (padded widths go dense) --; not ``compact_flag``
    (compact_as_of_node_flag); ``env_on`` -- HET_RGCN_BDD is not 0; not ``few_rels_dense`` -- R <= BDD_DENSE_UP_TO_RELS = 4 AND the
    dense two-call layer applies to the expansion (kernels.rgcn_layer_ok(R, K, D): all R dense weights in LDS).

    The last rule is measured (exp/rgcn_bdd_ab.py, profiles/r18/rgcn_bdd_ab.txt; MI355X, one layer 64 -> 64, B = 8, forward +
    backward medians of 200 interleaved steps): at the ogbn-mag shape, R = 4, native 1.11 + 1.46 ms against dense 0.84 + 1.15 ms --
    the dense layer's MFMA node pass with its four weights in LDS is 1.29x faster than the block products on the vector units, so
    such calls go dense.  At the AIFB size, R = 104, native 0.045 + 0.114 ms against 0.085 + 0.124 ms (0.76x); at the wikikg2
    size, R = 535, 5.03 + 6.90 ms against 5.25 + 6.87 ms (0.98x: a tie).  Nothing between R = 4 and R = 104 was timed: 5 <= R stays
    native, where the dense layer stops applying at R = 9 anyway (64 x 64)."""
    if cuda and fp32 and groupings and shape_ok and not compact_flag and env_on and not few_rels_dense:
        return "native"
    return "dense"


def rgcn_bdd_env_on() -> bool:
    return os.environ.get("HET_RGCN_BDD", "1") != "0"


def rgcn_bdd_route_of(graph, x, weight, norm, bias=None, compact_as_of_node_flag=False) -> str:
    """rgcn_bdd_route for these arguments."""
    R, nb, si, so = weight.shape
    fp32 = x.dtype == weight.dtype == norm.dtype == th.float32 and (bias is None or bias.dtype == th.float32)
    shape_ok = (x.dim() == 2 and x.shape[1] == nb * si and x.is_cuda and _k.rgcn_bdd_ok(R, nb * si, nb * so, nb) and
                x.shape[0] == graph.get_num_nodes() and (bias is None or bias.numel() == nb * so))
    # (HET_RGCN_BDD=native: the few-relations rule off -- what exp/rgcn_bdd_ab.py times at R = 4)
    few = bool(shape_ok and R <= BDD_DENSE_UP_TO_RELS and _k.rgcn_layer_ok(R, nb * si, nb * so) and
               os.environ.get("HET_RGCN_BDD") != "native")
    return rgcn_bdd_route(cuda=x.is_cuda, fp32=fp32, groupings=_k._plan.is_enabled(), shape_ok=shape_ok,
                          compact_flag=compact_as_of_node_flag, env_on=rgcn_bdd_env_on(), few_rels_dense=few)


@_consistent_plan
class RgcnLayerBdd(th.autograd.Function):
    """The RGCN layer with block-diagonal relation weights [R, B, si, so] as two library calls (include/het_amd.h:
    het_rgcn_bdd_layer_forward / _backward): RgcnLayerFused's dataflow with node passes and a weight gradient that multiply blocks.
    No gradient for norm (zeros when asked, as its neighbours)."""

    @staticmethod
    def forward(ctx, plan, x, weight, norm, bias):
        ret, ssum = _k.rgcn_bdd_layer_forward(plan, x, weight, norm, bias)
        ctx.plan, ctx.has_bias = plan, bias is not None
        ctx.save_for_backward(weight, norm, ssum)
        return ret

    @staticmethod
    def backward(ctx, gradout):
        weight, norm, ssum = ctx.saved_tensors
        grad_x, grad_w, grad_bias = _k.rgcn_bdd_layer_backward(
            ctx.plan, ssum, weight.transpose(2, 3).contiguous(), norm, gradout.float().contiguous(),
            ctx.has_bias and ctx.needs_input_grad[4], want_x=ctx.needs_input_grad[1])
        grad_norm = th.zeros_like(norm) if ctx.needs_input_grad[3] else None
        return None, grad_x, grad_w if ctx.needs_input_grad[2] else None, grad_norm, grad_bias


def rgcn_layer_bdd(graph, x, weight, norm, bias=None, compact_as_of_node_flag=False):
    """out [N, D] = bias + SUM_r SUM_{e: rel r, dst v} norm_e * x[src_e] . blockdiag(weight[r]);  weight [R, B, K/B, D/B].
    Routed by rgcn_bdd_route (rgcn_bdd_route_of tells which route these arguments take)."""
    if rgcn_bdd_route_of(graph, x, weight, norm, bias, compact_as_of_node_flag) == "native":
        s = graph.get_separate_coo_original()
        plan = _k.rgcn_bdd_layer_plan(s["rel_ptrs"], s["eids"], s["row_indices"], s["col_indices"], graph.get_num_nodes())
        if plan is None:
            raise _k._lib.HetError("rgcn_layer_bdd: the native route was chosen without groupings")
        return RgcnLayerBdd.apply(plan, x.contiguous(), weight.contiguous(), norm.contiguous(),
                                  None if bias is None else bias.contiguous())
    return rgcn_layer1_separate_coo(graph, x, bdd_dense_weight(weight), norm, bias)


@_consistent_plan
class _RGCNCompactAgg(th.autograd.Function):
    @staticmethod
    def forward(ctx, eids, rel_ptrs, row, col, map_a, map_b, feat_src, enorm, ret, direct):
        ctx.save_for_backward(eids, rel_ptrs, row, col, map_a, map_b, feat_src, enorm, ret)
        ctx.direct = direct
        d = {"inverse_indices_row": map_a} if direct else {"rel_ptrs_row": map_a, "node_indices_row": map_b}
        K.rgcn_node_mean_aggregation_compact_as_of_node_separate_coo(eids, rel_ptrs, row, col, d, feat_src, enorm, ret, direct)
        return ret

    @staticmethod
    def backward(ctx, gradout):
        eids, rel_ptrs, row, col, map_a, map_b, feat_src, enorm, ret = ctx.saved_tensors
        d = {"inverse_indices_row": map_a} if ctx.direct else {"rel_ptrs_row": map_a, "node_indices_row": map_b}
        grad_feat_src = th.zeros_like(feat_src, memory_format=th.contiguous_format)
        K.backward_rgcn_node_mean_aggregation_compact_as_of_node_separate_coo(
            eids, rel_ptrs, row, col, d, feat_src, enorm, ret, gradout.contiguous(), grad_feat_src, ctx.direct)
        return None, None, None, None, None, None, grad_feat_src, None, None, None


class RGCNNodeMeanAggregationCompactAsOfNodeSeparateCOO(th.autograd.Function):
    # reference: rgcn_layers_and_funcs.py:604-681
    @staticmethod
    def forward(ctx, separate_coo_eids, separate_coo_rel_ptrs, separate_coo_row_indices, separate_coo_col_indices,
                separate_unique_node_indices_rel_ptrs, separate_unique_node_indices_node_indices, feat_src, enorm, ret):
        raise RuntimeError("use .apply")

    @classmethod
    def apply(cls, eids, rel_ptrs, row, col, u_rel_ptrs, u_node_indices, feat_src, enorm, ret):  # noqa: D102
        return _RGCNCompactAgg.apply(eids, rel_ptrs, row, col, u_rel_ptrs, u_node_indices, feat_src, enorm, ret, False)


class RGCNNodeMeanAggregationCompactAsOfNodeDirectIndexingSeparateCOO(th.autograd.Function):
    # reference: rgcn_layers_and_funcs.py:684-754
    @staticmethod
    def forward(ctx, *a):
        raise RuntimeError("use .apply")

    @classmethod
    def apply(cls, eids, rel_ptrs, row, col, inverse_indices_row, feat_src, enorm, ret):  # noqa: D102
        return _RGCNCompactAgg.apply(eids, rel_ptrs, row, col, inverse_indices_row, inverse_indices_row, feat_src, enorm,
                                     ret, True)


def rgcn_node_mean_aggregation_compact_as_of_node_separate_coo_single_sided(g, feat_compact_src, enorm,
                                                                            compact_direct_indexing_flag):
    # reference: rgcn_layers_and_funcs.py:782-824
    s = g.get_separate_coo_original()
    ret = th.empty([g.get_num_nodes()] + list(feat_compact_src.size()[1:]), dtype=feat_compact_src.dtype,
                   device=feat_compact_src.device)
    if compact_direct_indexing_flag:
        inv = g.get_separate_unique_node_indices_single_sided_inverse_idx()
        return RGCNNodeMeanAggregationCompactAsOfNodeDirectIndexingSeparateCOO.apply(
            s["eids"], s["rel_ptrs"], s["row_indices"], s["col_indices"], inv["inverse_indices_row"],
            feat_compact_src.contiguous(), enorm.contiguous(), ret)
    ss = g.get_separate_unique_node_indices_single_sided()
    return RGCNNodeMeanAggregationCompactAsOfNodeSeparateCOO.apply(
        s["eids"], s["rel_ptrs"], s["row_indices"], s["col_indices"], ss["rel_ptrs_row"], ss["node_indices_row"],
        feat_compact_src.contiguous(), enorm.contiguous(), ret)
