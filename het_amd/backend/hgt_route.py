"""Which code serves a call of HET_HGTLayerHetero: ONE pure function of plain facts (``decide``) and the record it answers with
(``Route``).  het_amd/layers.py builds the facts and dispatches on ``Route.path``; hgt_fused_layer.py runs the ``fused`` path and
keeps the record on the autograd context of its attention node, where the backward reads its route from it.  No tensor, no graph
and no device is touched here, so the whole matrix is checked on the CPU (tests/test_hgt_route.py).

The paths, in the order ``decide`` tries them (the first row whose conditions hold is taken):

  path           served by                          conditions
  -------------  ---------------------------------  ----------------------------------------------------------------------------
  upcast         the fp32 layer on h.float(), the   a bf16 input that is not both FUSED_OK and NATIVE.  Correct, not faster.
                 result cast to bf16; the fp32
                 call is routed again
  fused          hgt_fused_layer.hgt_layer_fused    FUSED_OK
  weights_first  the layer's _forward_weights_first ``multiply_among_weights_first_flag``
  composition    the op-by-op code of layers.py     everything else

FUSED_OK: HET_HGT_FUSED on (``fused``), the groupings on (``plan``), a 2-d GPU tensor, a graph object with edges that has, or can
generate, the single-sided unique lists, a split of the heads into groups that the row kernels take (``groups``:
hgt_fused_layer._head_groups at the padded head width ``d_pad``), and relations that are canonical edge types (``canonical()``,
asked last: it reads the graph).
NATIVE (the bf16 kernels): a full graph (no ``typed_runs``), the padded input width and the row width H * d_pad both 32 or 64 -- one
head group and the shapes of rows_matmul_bf16_ok / rows_matmul_backward_split_ok follow -- and an output projection inside
rows_matmul_bf16_ok.

``fused`` records the widths (``Kp``, ``d_pad``, ``groups``, ``Xg``: the row width of one head group), ``native_bf16``, and
  compact_dst  q, new_h and the output projection on the destinations with in-edges only: those are fewer than
               ``compact_dst_below`` * N (``num_dst_rows()``)
  out_proj     bf16_rows (RowsLinearBf16) on the bf16 kernels; typed_gemm without compact destinations; with them rows_scatter
               (RowsLinearScatter) where rows_matmul_backward_split_ok takes the output width, else gemm_index_copy
  split_kv / split_q   rows_matmul_backward_split_ok of the attention node's two projections: separate dX / dW launches
  dx           the input gradient of the attention node: node_major (one pass over the nodes, csrc/node_sum.hip) on a full graph,
               ``Xg`` and ``Kp`` both 32 or 64, every node type within node_rows_matmul_sum_ok(1 + 2 * its outgoing relations)
               (``rels_per_type()``, asked last); else fp32_buffer for a bf16 input, per_relation for an fp32 one.
``composition`` and ``weights_first`` record ``score`` -- fused_score with ``hgt_fused_attn_score_flag``; else, on ``composition``
alone, compact with ``compact_as_of_node_flag``, or where the graph carries the single-sided lists (``lists_present``), on a GPU
tensor with the groupings on; else per_edge -- and ``direct`` = ``compact_direct_indexing_flag`` or not ``compact_as_of_node_flag``.
"""
from typing import Callable, List, NamedTuple, Optional

from .. import kernels as _k


class Facts(NamedTuple):
    """What ``decide`` reads about a call.  N: the rows of h; K_padded: the input width zero padding gives
    (layers._padded_in_width); (d_pad, groups): hgt_fused_layer._padded_head of the head width and _head_groups at it (None: no split
    fits); edges: a graph object (``graph_data``) with at least one edge; lists: it has, or can generate, the single-sided unique
    lists, lists_present: it has them; typed_runs: a sampled block whose nodes are runs of equal type (``node_segment_types``); the
    four ``*_flag`` fields: the reference's layer flags."""
    cuda: bool
    bf16: bool
    dim: int
    N: int
    K_padded: int
    H: int
    d_pad: int
    groups: Optional[int]
    out_dim: int
    plan: bool
    fused: bool               # hgt_fused_layer.FUSED
    edges: bool
    lists: bool
    lists_present: bool
    typed_runs: bool = False
    weights_first_flag: bool = False
    fused_attn_score_flag: bool = False
    compact_flag: bool = False
    direct_flag: bool = False
    compact_dst_below: float = 0.8   # hgt_fused_layer.COMPACT_DST_BELOW


class Route(NamedTuple):
    """The answer (the module docstring has every field)."""
    path: str
    Kp: Optional[int] = None
    d_pad: Optional[int] = None
    groups: Optional[int] = None
    Xg: Optional[int] = None
    native_bf16: bool = False
    compact_dst: bool = False
    out_proj: Optional[str] = None
    split_kv: bool = False
    split_q: bool = False
    dx: Optional[str] = None
    score: Optional[str] = None
    direct: bool = False


def decide(f: Facts, canonical: Callable[[], bool], num_dst_rows: Callable[[], int], rels_per_type: Callable[[], List[int]]) -> Route:
    """The route of a call (the table of the module docstring).  Supplied lazily, because each reads the graph: ``canonical()``,
    whether every relation has one source and one destination node type; ``num_dst_rows()``, the number of destinations with
    in-edges; ``rels_per_type()``, per node type the number of relations that leave it."""
    fused = f.fused and f.plan and f.cuda and f.dim == 2 and f.edges and f.lists and f.groups is not None
    native = bool(f.bf16 and not f.typed_runs and f.H * f.d_pad in (32, 64) and f.K_padded in (32, 64)
                  and _k.rows_matmul_bf16_ok(f.out_dim, f.out_dim))
    if not (fused and native == bool(f.bf16) and canonical()):
        if f.bf16:
            return Route("upcast")
        compact = not f.weights_first_flag and (f.compact_flag or (f.lists_present and f.cuda and f.plan))
        score = "fused_score" if f.fused_attn_score_flag else "compact" if compact else "per_edge"
        return Route("weights_first" if f.weights_first_flag else "composition", score=score, direct=f.direct_flag or not f.compact_flag)
    Kp, Xg = f.K_padded, f.H * f.d_pad // f.groups
    compact_dst = num_dst_rows() < f.compact_dst_below * f.N
    out_proj = ("bf16_rows" if native else "typed_gemm" if not compact_dst else
                "rows_scatter" if _k.rows_matmul_backward_split_ok(1, f.out_dim, f.out_dim) else "gemm_index_copy")
    node_major = (not f.typed_runs and Xg in (32, 64) and Kp in (32, 64)
                  and all(_k.node_rows_matmul_sum_ok(1 + 2 * n, Xg, Kp) for n in rels_per_type()))
    return Route("fused", Kp, f.d_pad, f.groups, Xg, native, compact_dst, out_proj,
                 split_kv=_k.rows_matmul_backward_split_ok(1, Kp, 2 * Xg), split_q=_k.rows_matmul_backward_split_ok(1, Kp, Xg),
                 dx="node_major" if node_major else "fp32_buffer" if f.bf16 else "per_relation")
