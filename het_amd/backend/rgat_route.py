"""Which code serves a call of HET_RGATLayer: ONE pure function of plain facts (``decide``) and the record it answers with
(``Route``).  het_amd/layers.py builds the facts and dispatches on ``Route.path``; rgat_fused_layer.py runs the four paths that
reach the library and keeps the record on the autograd context, where the backward reads its route from it.  No tensor, no graph and
no device is touched here, so the whole matrix is checked on the CPU (tests/test_rgat_route.py).

The paths, in the order ``decide`` tries them (the first row whose conditions hold is taken):

  path         served by                          conditions
  -----------  ---------------------------------  ------------------------------------------------------------------------------
  upcast       the fp32 layer on x.float(), the   a bf16 input that no row below serves natively: always with a halo; else unless
               result cast to bf16; the fp32      it is ``eval_bf16`` or ``train_bf16``.  Correct, not faster.
               call is routed again
  reference    reference_protocol                 ``reference_op_sequence`` (one GPU)
  composition  the op-by-op code of layers.py     ``gat_edge_parallel_flag`` off, ``op_by_op`` (HET_RGAT_FUSED=0; not looked at with
               (with a halo: not served, the      a halo), a halo without a self-loop, or no widths at which the one-node layer is
               caller exchanges first)            FUSED (below); with a halo also: not the distinct rows with er from the folded
                                                  weight, or widths outside rows_linear_bias_ok / rows_matmul_backward_split_ok
  eval         _forward_only                      FUSED, fp32, one GPU, no gradient can be asked for, HET_RGAT_FORWARD_ONLY on,
                                                  run sums (distinct rows, rgat_runs_shape_ok, N * R < 2^31)
  eval_bf16    _forward_only_bf16                 as ``eval`` for a bf16 input, in the shapes of rgat_bf16_shape_ok
  train_bf16   RgatLayerBf16Function              FUSED, bf16, one GPU, a gradient can be asked for, the layer's ``bf16_training``, the
                                                  shapes of rgat_bf16_shape_ok, N * R < 2^31, and a backward that is ``node_major``
                                                  with the attention gradient in the edge pass
  node         RgatLayerFunction                  FUSED, fp32, everything else (with or without a halo)

FUSED at widths (K', D') -- tried at the zero-padded widths first (HET_RGAT_PAD_HEADS on, padding that changes a width;
never with a halo), then at the layer's own: the groupings are on (het_amd.plan), a 2-d GPU tensor, slope >= 0, the graph has
edges, gat_grouped_shape_ok(H, D') (so a power-of-two number of heads and rows of at most 256 floats), a layer mulfirst flag only in
the shapes of the one-head row-dot; then, where the matrix-core projection takes the widths (matmul_attn_dot_ok): distinct rows, or
er from the folded weight, or matmul_attn_dot_only_ok's look at the lists -- elsewhere distinct rows AND the folded weight (the
any-shape GEMM + a row-dot for el).
Effective flags: distinct rows (``compact``, with direct indexing) whatever the layer flag says unless HET_RGAT_PER_EDGE or the
graph neither has nor can generate the single-sided lists; er from the folded weight (``mulfirst``) whatever the layer flag says
unless HET_RGAT_LITERAL_ER or the widths are outside the one-head row-dot; always on the bf16 paths.

The backward on distinct rows (``with_backward``; RgatLayerFunction._backward_distinct_rows has what each route does):
  node_major    er from the folded weight, the shapes of rgat_node_gemm_ok, every edge ending below nd
  per_relation  a halo, otherwise
  generic       one GPU, otherwise
and ``attn_in_pass`` (the gradient of attn_l from the edge pass): every route but ``generic``, run sums, at most 8 relations.
"""
from typing import Callable, NamedTuple, Optional

from .. import kernels as _k


class Facts(NamedTuple):
    """What ``decide`` reads about a call.  N: the rows of x the kernels see (with a halo: owned and halo rows, the nodes of the local
    graph); (K, D): the layer's own input and head widths; K_padded: the input width zero padding
    would give (layers._padded_in_width); grad: autograd is on and the input or a parameter requires a gradient; lists: the graph
    has, or can generate, the single-sided unique lists; the three ``*_flag`` fields: the reference's layer flags."""
    cuda: bool
    bf16: bool
    dim: int
    N: int
    K: int
    H: int
    D: int
    R: int
    K_padded: int
    edges: bool
    slope: float
    grad: bool
    halo: bool
    num_dst: Optional[int]
    plan: bool
    lists: bool
    compact_flag: bool = False
    direct_flag: bool = False
    mulfirst_flag: bool = False
    gat_edge_parallel: bool = True
    reference_op_sequence: bool = False
    op_by_op: bool = False
    self_loop: bool = False
    bf16_training: bool = False
    per_edge: bool = False      # rgat_fused_layer.PER_EDGE
    literal_er: bool = False    # rgat_fused_layer.LITERAL_ER
    forward_only: bool = True   # rgat_fused_layer.FORWARD_ONLY
    pad_heads: bool = True      # layers.PAD_HEADS


class Route(NamedTuple):
    """The answer.  (Kp, Dp): the widths the call runs with, the layer's own when nothing is padded.  ``backward`` / ``attn_in_pass``:
    of the paths with a backward on distinct rows; None / False until ``with_backward`` has resolved them (the bf16 node: in
    ``decide``; the fp32 node: when its backward runs)."""
    path: str
    R: int
    H: int
    Kp: int
    Dp: int
    compact: bool = False
    direct: bool = False
    mulfirst: bool = False
    run_sums: bool = False
    halo: bool = False
    backward: Optional[str] = None
    attn_in_pass: bool = False


def _mulfirst_shape_ok(H, Kd):
    """er = x[dst] . (W . attn_r) through the one-head row-dot kernels (seg_rowdot.hip)."""
    return H in (1, 2, 4, 8) and Kd >= 4 * H and Kd & (Kd - 1) == 0 and Kd <= 256


def _fused_flags(f: Facts, Kd, D, attn_dot_only):
    """The effective (compact, direct, mulfirst) of the one-node layer at widths (Kd, D), or None where it does not run there
    (FUSED in the module docstring)."""
    H = f.H
    if not (f.plan and f.cuda and f.dim == 2 and f.slope >= 0 and f.edges and _k.gat_grouped_shape_ok(H, D)):
        return None
    compact, direct, mulfirst = f.compact_flag, f.direct_flag, f.mulfirst_flag
    if mulfirst and not _mulfirst_shape_ok(H, Kd):
        return None
    if not compact and not f.per_edge and f.lists:
        compact, direct = True, True
    if not mulfirst and not f.literal_er and _mulfirst_shape_ok(H, Kd):
        mulfirst = True
    if _k.matmul_attn_dot_ok(H, Kd, D):
        ok = compact or mulfirst or attn_dot_only(f.R, H, Kd, D)
    else:
        # widths the matrix-core projection does not take (e.g. the 8 output classes of the reference CLI's defaults): the
        # distinct-row dataflow with er from the folded weight runs on the any-shape GEMM + a row-dot for el
        ok = compact and mulfirst
    return (compact, direct, mulfirst) if ok else None


def with_backward(route: Route, dst_prefix: Callable[[], bool]) -> Route:
    """``route`` with the route of its backward on distinct rows.  ``dst_prefix``: whether every edge ends below nd -- asked last,
    and only where the answer decides (the first time per graph it costs a device reduction and a host read)."""
    if not route.compact:
        return route
    node_major = route.mulfirst and _k.rgat_node_gemm_ok(route.R, route.H, route.Kp, route.Dp) and dst_prefix()
    backward = "node_major" if node_major else "per_relation" if route.halo else "generic"
    # (off the generic route the weight gradient of attn_l comes from the edge pass: csrc/gat_compact.hip ga_block_reduce)
    return route._replace(backward=backward, attn_in_pass=backward != "generic" and route.run_sums and route.R <= 8)


def decide(f: Facts, dst_below: Callable[[int], bool], attn_dot_only: Callable[[int, int, int, int], bool]) -> Route:
    """The route of a call (the table of the module docstring).  Supplied lazily, because each may read the graph's lists:
    ``dst_below(nd)``, whether every destination id is below nd, and ``attn_dot_only(R, H, K, D)``, kernels.matmul_attn_dot_only_ok
    at those widths."""
    R, H = f.R, f.H
    fallback = Route("upcast" if f.bf16 else "composition", R, H, f.K, f.D)
    if f.reference_op_sequence and not (f.bf16 or f.halo):
        return fallback._replace(path="reference")
    if (f.bf16 and f.halo) or f.reference_op_sequence or not f.gat_edge_parallel or (not f.self_loop if f.halo else f.op_by_op):
        return fallback
    widths = [(f.K, f.D)]
    if not f.halo and f.pad_heads:
        Dp = max(4, 32 // H, 1 << max(0, f.D - 1).bit_length())
        if (f.K_padded, Dp) != (f.K, f.D):
            widths.insert(0, (f.K_padded, Dp))
    for Kp, Dp in widths:
        flags = _fused_flags(f, Kp, Dp, attn_dot_only)
        if flags is not None:
            break
    else:
        return fallback
    compact, direct, mulfirst = flags
    # (run sums: the shapes of the run-sum form, and destination * R + relation inside the groupings' int32 keys -- else
    #  kernels.rgat_compact_groupings builds the per-edge form, whatever the forward asks for)
    run_sums = compact and _k.rgat_runs_shape_ok(H, Dp) and f.N * R < 2 ** 31
    node = Route("node", R, H, Kp, Dp, compact, direct, mulfirst, run_sums, f.halo)
    if f.halo:
        served = compact and mulfirst and _k.rows_linear_bias_ok(Kp, H * Dp) and _k.rows_matmul_backward_split_ok(H, Kp, Dp)
        return node if served else fallback
    evaluation = f.forward_only and not f.grad and run_sums
    if not f.bf16:
        return node._replace(path="eval") if evaluation else node
    if not (run_sums and _k.rgat_bf16_shape_ok(H, Kp, Dp)):
        return fallback
    native = node._replace(mulfirst=True)  # (the literal er needs a second projection table: there is no bf16 form of it)
    if evaluation:
        return native._replace(path="eval_bf16")
    if f.grad and f.bf16_training:
        # (the shapes of rgat_node_gemm_ok -- at most 8 relations, K and H * D' each 32 or 64 -- are inside rows_matmul_bf16_ok's)
        nd = f.N if f.num_dst is None else min(int(f.num_dst), f.N)
        trained = with_backward(native._replace(path="train_bf16"), lambda: dst_below(nd))
        if trained.attn_in_pass:  # (one GPU: on the node_major route, then)
            return trained
    return fallback
