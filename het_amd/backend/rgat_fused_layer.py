"""The whole RGAT layer (RGAT/models.py:16-385) as ONE autograd node.

Same ops, same values and gradients as the op-by-op composition in het_amd/layers.py (which follows the reference's
model code and stays the fallback); what the single node buys is control over the backward pass: every consumer of the
layer input accumulates its gradient into ONE buffer (self-loop first with plain stores, then the two projections with
their atomic epilogues) and the weight gradients into one buffer, instead of autograd allocating a gradient per
consumer and summing them with elementwise kernels; the output ``h + loop_message + h_bias`` is one pass.  On ogbn-mag
this removes ~1 ms of elementwise adds and fills per step.

Two dataflows:
  distinct rows (kinds 3 / 4)   projections on the unique (relation, node) rows, gathered by the GAT kernels through the
                           (relation, source) -> row map; el folded into the compact GAT backward.  This is what the
                           reference's --compact_as_of_node_flag selects AND what the default flags run on here: inside
                           one autograd node no per-edge tensor is visible to the caller, the values are the same
                           (feat_src_per_edge[e] == feat_compact[row(e)] bit for bit), and the [E,H,D] tensor and its
                           gradient (5.4 GB each on ogbn-mag) are never written.  The unique lists are the ones the
                           reference's RGAT script builds for every run (RGAT/train_dgl.py:160, unconditional); a graph
                           that lacks them gets them from the device-side builders once.
  per edge (kind 0)        the round-1 dataflow of the default flags: [E,H,D] projections (distinct-row projection +
                           broadcast), el / er / exp / grad_el in the destination-grouped order of the GAT kernels.  Kept
                           behind HET_RGAT_PER_EDGE=1 for A/B runs and as the path tests/ compare the other with.
and, for either, ``mulfirst`` (--multiply_among_weights_first_flag, RGAT/models.py:300-326): er = x[dst] . (W . attn_r)
as a row-dot product on the distinct (relation, destination) rows instead of a projection followed by a dot.  The two
forms of er are the same real number (associativity); the reference offers the flag because it is cheaper, and so the
node takes it whenever the one-head row-dot kernels cover the shape (HET_RGAT_LITERAL_ER=1 keeps (x . W) . attn_r).

Which of the functions below serves a call -- and which dataflow, which form of er, which route of the backward -- is decided once
per call, by rgat_route.decide: the table of its module docstring has every path with its conditions.  rgat_layer_fused runs the
record it is handed (``Route``), the autograd nodes keep it on their context.

The backward of the distinct-row dataflow is ONE function for one GPU and for a partition with a halo
(RgatLayerFunction._backward_distinct_rows): its routes differ in how the input gradient is formed, nothing else.

Evaluation (path ``eval``) does not go through the node at all: _forward_only runs the same forward with an aggregation that keeps
nothing for a backward.

bf16 activations (a torch.bfloat16 input) on the evaluation path (``eval_bf16``): _forward_only_bf16 keeps x, feat_c and the layer
output h as bf16 rows, each rounded once (to nearest even) where its kernel stores it; W, attn_l, attn_r, the self-loop weight, the
bias, el_c, er_c, the hub records and every sum, maximum and exponential are fp32 on widened values.  er always comes from the
folded weight there, and el_c is the dot of the ROUNDED feat_c row, so the walks that form el from the row they gather and those
that gather el_c compute one function.

bf16 training (``train_bf16``): RgatLayerBf16Function runs that same forward with the training aggregation over bf16 rows -- it also
leaves lse, ret [N,H,D], the run sums and el_c, all fp32 -- and its backward is the node-major route of _backward_distinct_rows with
the bf16 entries: the incoming gradient of h is gathered as bf16 rows and widened on load, grad_feat_c / grad_er_c and every
parameter gradient are fp32 sums, the gradient passes straight through the rounding of feat_c, and grad_x is rounded once where the
node-major pass stores a node's finished row.  No fp32 copy of x, feat_c, h, grad_h or grad_x is made.

Attention weights (the layer's get_attention=True): both evaluation functions append attn [E,H] (fp32, edge-id order) to the list
they are handed -- a pass over the ids, el_c and er_c after the aggregation (csrc/gat_attention.hip); the autograd node does not, and
the layer composes them in torch (attention_composition): correct, not fast.
"""
import os

import torch as th

from ..plan import consistent as _consistent_plan

from .. import kernels as _k
from ..kernels import K
from . import rgat_route


_OFFS = {}
PER_EDGE = os.environ.get("HET_RGAT_PER_EDGE") == "1"      # default flags on the per-edge (kind 0) dataflow
LITERAL_ER = os.environ.get("HET_RGAT_LITERAL_ER") == "1"  # er = (x . W) . attn_r unless the layer flag asks otherwise
OVERLAP = os.environ.get("HET_RGAT_OVERLAP", "1") != "0"  # independent launches on a second HIP stream (see _side_stream)
FORWARD_ONLY = os.environ.get("HET_RGAT_FORWARD_ONLY", "1") != "0"  # no backward in sight: the forward that keeps nothing for one


def _has_single_sided_lists(g):
    return "unique_node_indices_single_sided" in getattr(g, "graph_data", {}).get("separate", {})


def _destinations_below(col, nd):
    """Whether every destination id is < nd (cached per graph: one reduction + host read the first time)."""
    return col.numel() == 0 or _k._derived_get("col_max", (col,), lambda: int(col.max())) < nd


def _lists(g):
    s = g.get_separate_coo_original()
    by_src = {"separate_coo_rel_ptrs": s["rel_ptrs"], "separate_coo_node_indices": s["row_indices"], "separate_coo_eids": s["eids"]}
    by_dst = {"separate_coo_rel_ptrs": s["rel_ptrs"], "separate_coo_node_indices": s["col_indices"], "separate_coo_eids": s["eids"]}
    return s, by_src, by_dst


def _eids_are_positions(eids):
    """Whether eids[p] == p for every position (what canonicalize_eids leaves; checked once per list)."""
    return _k._derived_get("eids_are_positions", (eids,),
                           lambda: bool((eids == th.arange(eids.numel(), device=eids.device)).all()))


def _edge_rows(g, ss, direct, rp, row, col, eids):
    """(feat row, er row) of every edge position, [E] int64 each: the graph's inverse indices when it carries them
    (indexed by edata id == position after canonicalize_eids), else located in the unique lists once and cached."""
    sep = getattr(g, "graph_data", {}).get("separate", {}).get("unique_node_indices_single_sided", {})
    if "inverse_indices_row" in sep and getattr(g, "sequential_eids_format", None) == "separate_coo":
        if _eids_are_positions(eids):
            return sep["inverse_indices_row"], sep["inverse_indices_col"]
        # (edge ids renumbered after the lists were built: the inverse indices are read by edge id)
        maps = (sep["inverse_indices_row"], None, sep["inverse_indices_col"], None)
        return _k._src_rows_by_position(4, maps, rp, row, eids), _k._dst_rows_by_position(4, maps, rp, col, eids)
    maps = (ss["rel_ptrs_row"], ss["node_indices_row"], ss["rel_ptrs_col"], ss["node_indices_col"])
    return _k._src_rows_by_position(3, maps, rp, row, eids), _k._dst_rows_by_position(3, maps, rp, col, eids)


def rgat_layer_fused_ok():
    """The ``plan`` fact of rgat_route.decide: the groupings are on (het_amd.plan), without which nothing in this module runs.
    (Tests replace it with a constant False: the op-by-op composition of layers.py with the groupings still on.)"""
    return _k._plan.is_enabled()


def graph_facts(g, x):
    """What rgat_route.decide is told about the graph, (lists, dst_below, attn_dot_only): whether it has, or can generate, the
    single-sided unique lists, and the two facts that may read its lists, as callables for decide to ask where they matter."""
    lists = _has_single_sided_lists(g) or hasattr(g, "generate_separate_unique_node_indices_single_sided_for_each_etype")
    dst_below = lambda nd: _destinations_below(g.get_separate_coo_original()["col_indices"], nd)
    attn_dot_only = lambda R, H, Kd, D: _k.matmul_attn_dot_only_ok(_lists(g)[2], th.empty((R, H, Kd, D), device="meta"), x)
    return lists, dst_below, attn_dot_only


_SIDE = {}


def _side_stream(dev):
    """A second HIP stream per device for launches that do not depend on each other and are bound by different units: the
    weight-gradient passes (HBM-bound: they stream x / feat_c / gradient rows once) beside the node-major input-gradient pass
    (matrix-core-bound), the self-loop GEMM (HBM-bound) beside the projection GEMM.  The caller brackets the side work with
    events: it starts after everything it reads and the main stream waits for it before anything reads its outputs (or frees
    its inputs), so the allocator never sees a cross-stream use.
    Everything the side stream WRITES is allocated before the fork (``side.wait_stream(main)``): a block handed out later may
    have been freed by a tensor whose last main-stream kernel was enqueued after the fork -- the side stream would not wait
    for it.
    Everything the side stream READS that no output of the step keeps alive stays referenced until the join
    (``main.wait_stream(side)``) has been enqueued: the workspace of the backward's edge pass, whose partial rows of grad_attn_l the
    side stream sums (kernels.rgat_attn_grad_finish) -- released earlier, its block could go to a main-stream allocation made
    between the fork and the join, and that tensor's kernels would not wait for the side stream's read.
    What runs there, per step: forward -- the er row-dot and the self-loop GEMM beside the projection;
    backward -- the self-loop's weight gradient beside the gather passes (first fork), then the attention-gradient finish and the
    weight gradients of W and W.attn_r beside the node-major pass (second fork)."""
    s = _SIDE.get(dev)
    if s is None:
        s = _SIDE[dev] = th.cuda.Stream(device=dev)
    return s


def _unique_lists(g):
    """(ss, d_row, d_col): the graph's unique (relation, source) / (relation, destination) lists and the argument dictionaries
    (kind 1) of the relational products over either."""
    ss = g.get_separate_unique_node_indices_single_sided()
    d_row = {"unique_srcs_and_dests_rel_ptrs": ss["rel_ptrs_row"], "unique_srcs_and_dests_node_indices": ss["node_indices_row"]}
    d_col = {"unique_srcs_and_dests_rel_ptrs": ss["rel_ptrs_col"], "unique_srcs_and_dests_node_indices": ss["node_indices_col"]}
    return ss, d_row, d_col


def _folded_weight(W, attn_r):
    """wa[r,h,k] = SUM_d W[r,h,k,d] * attn_r[r,h,d] (RGAT/models.py:300-326): the attention vector folded into the weight, as the
    one-input-head weight [R,H,K,1] of the relational products; its transpose [R,H,1,K] and the rows [R,H,K] of the row-dot and
    node-major kernels are views of the same memory.  Once per step, in the forward; the backward takes it from the context."""
    R, H, Kd, D = W.shape
    return th.bmm(W.view(-1, Kd, D), attn_r.view(-1, D, 1)).view(R, H, Kd, 1)


def _unfold_weight_gradient(grad_wa, W, attn_r, grad_W):
    """The gradient through _folded_weight: grad_W += grad_wa (x) attn_r in place; returns grad_attn_r.  grad_wa [R,H,K,1].  One
    launch, sums in a fixed order (csrc/node_gemm.hip: HET_rgat_unfold_weight_gradient)."""
    return _k.rgat_unfold_weight_gradient(grad_wa, W, attn_r, grad_W)


def _gradients(grad_x, grad_W, grad_attn_l, grad_attn_r, grad_loop, grad_bias):
    """What RgatLayerFunction.backward returns: nothing for (g, route, slope, num_dst, halo)."""
    return None, None, None, None, None, grad_x, grad_W, grad_attn_l, grad_attn_r, grad_loop, grad_bias


def _halo_pieces(g, ss, plan):
    """The unique (relation, source) list of a partition's local graph cut by when the source node's row of x is there: the
    owned nodes together with piece 0 of the halo exchange, then every further piece (local ids n_own + halo_chunk_ptr[c] ..).
    Per cut a relation-bucketed list (rel_ptrs [R+1], node ids, row index in the full list), built once per graph."""
    key = ("halo_pieces", plan.chunks, plan.n_own, plan.n_halo)
    hit = g._plans.get(key)
    if hit is None:
        with _k._plan.building():  # (kept on the graph: normal tensors whatever the caller's mode)
            hit = g._plans[key] = _build_halo_pieces(ss, plan)
    return hit


def _build_halo_pieces(ss, plan):
    rp_row, nodes = ss["rel_ptrs_row"], ss["node_indices_row"]
    R = rp_row.numel() - 1
    rel = th.repeat_interleave(th.arange(R, device=nodes.device), rp_row[1:] - rp_row[:-1])
    # (the owned sources -- 5 % of a rank's rows on ogbn-mag at 8 ranks -- go with the first piece: a launch less per step, and
    #  a rank's step at 8 ranks is short enough for every launch to count, profiles/r04/dist_rank_share_halo.txt)
    cuts = [(0, plan.n_own + plan.halo_chunk_ptr[1])] + [(plan.n_own + plan.halo_chunk_ptr[c], plan.n_own + plan.halo_chunk_ptr[c + 1])
                                                         for c in range(1, plan.chunks)]
    hit = []
    for a, b in cuts:
        sel = th.nonzero((nodes >= a) & (nodes < b)).flatten()  # ascending: still relation-major
        rp_c = th.zeros(R + 1, dtype=th.int64, device=nodes.device)
        rp_c[1:] = th.cumsum(th.bincount(rel[sel], minlength=R), 0)
        hit.append((rp_c, nodes[sel].contiguous(), sel.contiguous()))
    assert sum(int(h[2].numel()) for h in hit) == nodes.numel()
    return hit


def _loop_offsets(nd, device):
    """[0, nd] int64 on the device: the one-relation pointer list of the self-loop product (built once per (rows, device): no
    per-step host-to-device copy)."""
    offs = _OFFS.get((nd, device))
    if offs is None:
        if len(_OFFS) > 64:
            _OFFS.clear()
        with _k._plan.building():  # (kept for later calls, whose autograd nodes save it: a normal tensor whatever the caller's mode)
            offs = _OFFS[(nd, device)] = th.tensor([0, nd], dtype=th.int64, device=device)
    return offs


def _prologue(x, W, attn_l, attn_r, loop_w, num_dst, halo=None):
    """What every forward starts with: contiguous operands, the destination rows nd and the self-loop's pointer list.  Returns
    (x, W, attn_l, attn_r, loop_w, nd, offs)."""
    x, W, attn_l, attn_r = x.contiguous(), W.contiguous(), attn_l.contiguous(), attn_r.contiguous()
    if halo is not None:
        # multi-GPU (het_amd/dist.py): x holds the owned rows; the halo rows of x_local arrive through an all-to-all
        # that is in flight until halo.finish_push() -- everything before that reads owned rows only
        x = halo.start_push(x)
    N = x.shape[0]
    nd = N if num_dst is None else min(int(num_dst), N)
    offs = None
    if loop_w is not None:
        loop_w = loop_w.contiguous()
        offs = _loop_offsets(nd, x.device)
    return x, W, attn_l, attn_r, loop_w, nd, offs


def _loop_and_bias_rows(rows, x, nd, offs, loop_w, bias):
    """Without fused self-loop rows for the aggregation to add into (no self-loop, or widths its fused launch does not take):
    ``rows`` + x[:nd] . loop_w + bias as a product and an add of their own; None when there is neither term."""
    if loop_w is None and bias is None:
        return None
    loop = None
    if loop_w is not None:
        loop = x.new_empty((nd, loop_w.shape[1]))
        K.rgnn_relational_matmul_no_scatter_gather_list(offs, loop_w.view(1, 1, *loop_w.shape), x[:nd], loop)
    return _k.rows_add_bias(rows, loop, None if bias is None else bias.contiguous())


def _compact_tables(g, direct, mulfirst, halo, nd, offs, x, W, attn_l, attn_r, loop_w, bias, for_backward=False):
    """The distinct-row forward in front of its aggregation, common to RgatLayerFunction.forward and _forward_only: the
    projections feat_c / el_c / er_c on the unique (relation, node) rows, the self-loop + bias rows ``h`` the aggregation adds into
    (None when there is no self-loop or its fused launch does not take the widths) and the groupings of the edges.  Returns
    (ss, h, saved, grp, run_sums, forms); saved = (feat_c, el_c, er_c[, feat_d]).
    ``forms`` = (W^T [R,H,D,K], loop_w^T [X,K] or None, wa [R,H,K,1] or None), the forms of the parameters the step's kernels read:
    the folded weight wa (``mulfirst``), once per step; the transposes -- ``for_backward`` alone, else None: only the backward reads
    them -- as one launch behind the projection, on the stream that has slack there (the projection ends before the self-loop's
    launch beside it does: profiles/r11/default_timeline_after.txt)."""
    s, _, _ = _lists(g)
    rp, row, col, eids = s["rel_ptrs"], s["row_indices"], s["col_indices"], s["eids"]
    N = x.shape[0]
    R, H, Kd, D = W.shape
    X = H * D
    new = lambda *shape: th.empty(shape, dtype=x.dtype, device=x.device)
    h = None
    ss, d_row, d_col = _unique_lists(g)
    featc = new(ss["node_indices_row"].numel(), H, D)
    elc = new(featc.shape[0], H)
    erc = new(ss["node_indices_col"].numel(), H)
    # (the destination side and the self-loop read rows of destination nodes only -- owned rows on a partition)
    side = None
    fused_loop = loop_w is not None and _k.rows_linear_bias_ok(Kd, X)
    # (the three products below read the same rows of x; one node-major pass that reads them once was built and measured in
    #  round 5 -- 1 GB less traffic, the same step time: exp/node_fwd.hip.txt)
    if OVERLAP and halo is None and fused_loop and mulfirst:
        # er_c (a row-dot) and the self-loop GEMM are HBM-bound streams of rows: on the side stream beside the projection
        main, side = th.cuda.current_stream(x.device), _side_stream(x.device)
        h = x.new_empty((nd, X))  # (with erc above: what the side stream writes, allocated before the fork -- _side_stream)
    # (in front of the fork: on the side stream, in front of its one reader here, the bmm's 16 workgroups waited 0.09 ms for a
    #  slot behind the projection's 1 857 and the row-dot started that much later -- DESIGN.md 4.2)
    wa = _folded_weight(W, attn_r) if mulfirst else None
    if side is not None:
        side.wait_stream(main)
    if mulfirst:
        with th.cuda.stream(side if side is not None else th.cuda.current_stream(x.device)):
            K.rgnn_relational_matmul(d_col, 1, wa, x, erc.view(-1, H, 1), True)
        saved = (featc, elc, erc)
    else:
        featd = new(erc.shape[0], H, D)
        _k.matmul_attn_dot(d_col, 1, W, x, featd, attn_r, erc)
        saved = (featc, elc, erc, featd)
    if fused_loop:
        # self-loop + bias first (bias in the GEMM epilogue); the aggregation adds its rows into h in place: no
        # separate h = ret + loop + bias pass and no zero fill of ret (read by the backward only where edges point)
        bias_c = None if bias is None else bias.contiguous()
        if side is not None:  # (h: allocated, and later freed, under the main stream; the side stream only fills it)
            with th.cuda.stream(side):
                _k.rows_linear_bias(offs, x[:nd], loop_w, bias_c, out=h)
        else:
            h = _k.rows_linear_bias(offs, x[:nd], loop_w, bias_c)
    dot_ok = _k.matmul_attn_dot_ok(H, Kd, D)
    piecewise = halo is not None and halo.chunks > 1 and dot_ok
    if halo is not None and not piecewise:
        halo.finish_push()
    if piecewise:
        # the exchange arrives in pieces (het_amd/dist.py: DistPlan.chunks): the rows whose source node is owned are
        # projected at once, the rows of piece c as soon as piece c is there -- piece c + 1 is on the wire meanwhile
        for c, (rp_c, nodes_c, rows_c) in enumerate(_halo_pieces(g, ss, halo.plan)):
            halo.wait_push_piece(c)
            _k.matmul_attn_dot_rows(rp_c, nodes_c, rows_c, W, x, featc, attn_l, elc)
        halo.finish_push()
    elif dot_ok:
        _k.matmul_attn_dot(d_row, 1, W, x, featc, attn_l, elc)  # el_c = <feat_c, attn_l[r]> from the GEMM epilogue
    else:  # other widths: any-shape projection, then el_c as a row-dot over the relation-bucketed rows
        K.rgnn_relational_matmul(d_row, 1, W, x, featc, True)
        K.rgnn_relational_matmul_no_scatter_gather_list(ss["rel_ptrs_row"], attn_l.unsqueeze(-1), featc, elc.view(-1, H, 1))
    Wt, loop_wt = _k.rgat_transpose_weights(W, loop_w) if for_backward else (None, None)
    if side is not None:
        th.cuda.current_stream(x.device).wait_stream(side)
    # edge softmax + aggregation straight from the compact tables: no exp [E,H] tensor (csrc/gat_compact.hip)
    srow, drow = _edge_rows(g, ss, direct, rp, row, col, eids)
    # (run sums: grad_er from S_col rows the forward leaves instead of a per-edge term -- csrc/gat_compact.hip)
    run_sums = _k.rgat_runs_shape_ok(H, D)
    grp = _k.rgat_compact_groupings(col, srow, drow, N, featc.shape[0], erc.shape[0], rel_ptrs=rp if run_sums else None,
                                    drow_nodes=ss["node_indices_col"], drow_rel_ptrs=ss["rel_ptrs_col"])
    return ss, h, saved, grp, run_sums, (Wt, loop_wt, wa)


def _per_relation_front(x, loop_w, offs, grad_h, nd, H, dst_prefix):
    """What the two backwards that add the input gradient relation by relation (generic distinct rows, per edge) start with.
    Returns (grad_x, grad_loop, go): ONE input-gradient buffer -- the self-loop writes its rows with plain stores (and its weight
    gradient from the same launch), the projections add to it -- and the output gradient per destination row."""
    N, Kd = x.shape
    X = grad_h.shape[1]
    grad_loop = None
    if loop_w is not None:
        grad_x = th.empty_like(x) if nd == N else th.zeros_like(x)
        grad_loop = th.empty_like(loop_w)
        _k.matmul_no_scatter_gather_backward(offs, loop_w.view(1, 1, Kd, X).transpose(2, 3).contiguous(), x[:nd], grad_h,
                                             grad_x[:nd], grad_loop.view(1, 1, Kd, X), accumulate=False)
    else:
        grad_x = th.zeros_like(x)
    if nd == N or dst_prefix:
        go = grad_h.view(nd, H, X // H)
    else:  # rows of non-destination nodes receive no gradient
        go = th.zeros((N, H, X // H), dtype=x.dtype, device=x.device)
        go.view(N, X)[:nd] = grad_h
    return grad_x, grad_loop, go


@_consistent_plan
class RgatLayerFunction(th.autograd.Function):
    @staticmethod
    def forward(ctx, g, route, slope, num_dst, halo, x, W, attn_l, attn_r, loop_w, bias):
        compact, direct, mulfirst = route.compact, route.direct, route.mulfirst
        x, W, attn_l, attn_r, loop_w, nd, offs = _prologue(x, W, attn_l, attn_r, loop_w, num_dst, halo)
        s, by_src, by_dst = _lists(g)
        rp, row, col, eids = s["rel_ptrs"], s["row_indices"], s["col_indices"], s["eids"]
        E, N = eids.numel(), x.shape[0]
        R, H, Kd, D = W.shape
        X = H * D
        new = lambda *shape: th.empty(shape, dtype=x.dtype, device=x.device)
        sm, ret = new(N, H), new(N, H, D)
        h = None
        if compact:
            ss, h, saved, grp, run_sums, ctx.forms = _compact_tables(g, direct, mulfirst, halo, nd, offs, x, W, attn_l, attn_r, loop_w, bias,
                                                                      for_backward=True)
            featc, elc, erc = saved[:3]
            # (elc IS <featc, attn_l[relation of the row]>: the pass may form it from the rows it gathers -- kernels.py)
            ctx.runs = _k.rgat_aggregate_compact(grp, featc, elc, erc, sm, ret, slope, h_inout=h, num_rels=R,
                                                 attn_l=attn_l.contiguous() if run_sums else None, feat_rel_ptrs=ss["rel_ptrs_row"] if run_sums else None)
            ctx.grp = grp
            ex = x.new_empty(0)
        else:
            # el / er are produced directly in the destination-grouped order of the GAT kernels (rank of every position):
            # the aggregation pass forms exp from two coalesced streams, no exp pass, no per-edge 16-byte gathers
            rank = _k.gat_rank_of_position(rp, row, col, eids, N)
            by_dst_s = {"separate_coo_rel_ptrs": rp, "separate_coo_node_indices": col, "separate_coo_eids": rank}
            feat, el_s, er_s, exs = new(E, H, D), new(E, H), new(E, H), new(E, H)
            _k.matmul_attn_dot(by_src, 0, W, x, feat, attn_l, el_s, dot_rows=rank)
            if mulfirst:
                K.rgnn_relational_matmul(by_dst_s, 0, _folded_weight(W, attn_r), x, er_s.view(E, H, 1), True)
                saved = (feat, exs)
            else:
                comp = _k.matmul_attn_dot(by_dst_s, 0, W, x, None, attn_r, er_s)
                assert comp is not None
                saved = (feat, exs, comp)
            used = _k.fused_gat_forward(eids, rp, row, col, 0, {}, feat, None, None, sm, None, ret, slope, exs,
                                        el_sorted=el_s, er_sorted=er_s)
            assert used
            ex = x.new_empty(0)
        if h is None:
            out = ret.view(N, X)[:nd]
            h = _loop_and_bias_rows(out, x, nd, offs, loop_w, bias)
            if h is None:
                h = out.clone()
        ctx.halo = halo
        ctx.g, ctx.route, ctx.slope, ctx.nd = g, route, slope, nd
        ctx.has_loop, ctx.has_bias = loop_w is not None, bias is not None
        ctx.save_for_backward(x, W, attn_l, attn_r, loop_w if loop_w is not None else x.new_empty(0), offs if offs is not None else eids,
                              sm, ex, ret, *saved)
        return h

    @staticmethod
    def backward(ctx, grad_h):
        grad_h = grad_h.contiguous()
        if ctx.route.compact:
            return RgatLayerFunction._backward_distinct_rows(ctx, grad_h)
        x, W, attn_l, attn_r, loop_w, offs, sm, ex, ret, *saved = ctx.saved_tensors
        g, nd, slope = ctx.g, ctx.nd, ctx.slope
        s, by_src, by_dst = _lists(g)
        rp, row, col, eids = s["rel_ptrs"], s["row_indices"], s["col_indices"], s["eids"]
        N, Kd = x.shape
        E = eids.numel()
        R, H, _, D = W.shape
        grad_bias = grad_h.sum(0) if ctx.has_bias else None
        Wt = th.transpose(W, 2, 3).contiguous()
        grad_W = th.zeros_like(W)
        grad_x, grad_loop, go = _per_relation_front(x, loop_w if ctx.has_loop else None, offs, grad_h, nd, H, False)
        mulfirst = ctx.route.mulfirst
        if mulfirst:
            wa_t = _folded_weight(W, attn_r).view(R, H, 1, Kd)
            grad_wa = th.zeros((R, H, Kd, 1), dtype=x.dtype, device=x.device)
        feat, exs = saved[:2]
        # the edges' grad_el (= grad_er) in the kernel's destination-grouped order: sequential stores, and the
        # (relation, destination) sums of the er side read contiguous runs instead of scattered 16-byte pieces
        rank = _k.gat_rank_of_position(rp, row, col, eids, N)
        by_dst = {"separate_coo_rel_ptrs": rp, "separate_coo_node_indices": col, "separate_coo_eids": rank}
        g_feat, g_el = th.empty_like(feat), th.empty_like(exs)
        grad_attn_l = th.zeros_like(attn_l)
        if R <= 8:
            _k.fused_gat_backward(eids, rp, row, col, 0, {}, feat, None, None, sm, None, ret, go, g_feat, None, None, slope,
                                  exs, fold_attn_l=attn_l, grad_fold_attn_l=grad_attn_l, grad_el_sorted=g_el)
        else:
            g_el_e = th.empty_like(exs)
            _k.fused_gat_backward(eids, rp, row, col, 0, {}, feat, None, None, sm, None, ret, go, g_feat, g_el_e, g_el_e, slope,
                                  exs, fold_attn_l=attn_l, grad_el_sorted=g_el)
            by_eid = {"separate_coo_rel_ptrs": rp, "separate_coo_node_indices": eids, "separate_coo_eids": eids}
            _k.matmul_backward(by_eid, 0, attn_l.unsqueeze(2), feat, g_el_e, None, grad_attn_l.unsqueeze(-1), False,
                               accumulate=False)
        _k.matmul_backward(by_src, 0, Wt, x, g_feat, grad_x, grad_W, True, accumulate=True)
        if mulfirst:
            _k.matmul_backward(by_dst, 0, wa_t, x, g_el.view(E, H, 1), grad_x, grad_wa, True, accumulate=True)
            grad_attn_r = _unfold_weight_gradient(grad_wa, W, attn_r, grad_W)
        else:
            grad_attn_r = th.zeros_like(attn_r)
            ok = _k.matmul_attn_dot_only_backward(by_dst, Wt, x, attn_r, g_el, grad_x, grad_W, comp_rows=saved[2],
                                                  grad_dot_w=grad_attn_r, accumulate=True)
            assert ok, "the grouping of the forward pass is gone"
        return _gradients(grad_x, grad_W, grad_attn_l, grad_attn_r, grad_loop, grad_bias)

    @staticmethod
    def _backward_distinct_rows(ctx, grad_h):
        """The backward on the distinct-row dataflow, on one GPU and on a partition.  One edge pass (rgat_backward_compact) leaves
        the gradients of the compact tables; what differs between the routes is how the input gradient is formed from them:
          node-major              every term of grad_x gathered per node (csrc/node_gemm.hip): one pass stores grad_x (self-loop +
                                  relation projections + the folded attention vector) -- instead of a self-loop pass and one
                                  read-modify-write launch per relation and side.  er from the folded weight, the shapes of
                                  het_rgat_node_gemm_ok, every edge ending below nd.
          node-major, partition   the same pass per node range, ordered around the reverse halo exchange: the halo rows first --
                                  only the (relation, source) projections reach them -- so that they leave with an all-to-all
                                  while the owned rows and the weight gradients are formed; the returned rows are added to the
                                  owners' gradients at the end.
          per relation            the self-loop stores its rows of grad_x, the projections add theirs relation by relation: a
                                  partition at the other matrix-core shapes (split launches: input gradient, then weight
                                  gradients), and every other call (``generic``: any shape, literal er, edges ending at or above
                                  nd -- launches that form an input and a weight gradient together, "+=").
        On all but the generic route the weight gradients are launches of their own, HBM-bound streams of rows: on the side stream
        beside the gather passes and the matrix-core-bound node pass; the self-loop's needs x and grad_h only and starts at once.
        Nothing that depends on the parameters alone is made here: W^T, loop_w^T and the folded weight wa come from the forward
        (ctx.forms, _compact_tables) -- as launches of the backward they stood where the whole chip waited for them, in front of the
        edge pass and between it and the node-major pass.  On the node-major routes with the side stream the edge pass also leaves
        the sum of grad_attn_l's partial rows to the side stream (after the second fork, in front of the weight gradients): the
        node-major pass starts where the edge pass ends.  The fold of grad_wa back into grad_W / grad_attn_r behind the last join is
        one launch (_unfold_weight_gradient).
        bf16 rows (RgatLayerBf16Function: x, feat_c and grad_h bf16): the node-major route alone, with the bf16 entries; every
        gradient table and parameter gradient is fp32, grad_x bf16."""
        x, W, attn_l, attn_r, loop_w, offs, sm, _, ret, featc, elc, erc, *featd = ctx.saved_tensors
        # (the forms of the parameters the forward made for this step: W^T [R,H,D,K], loop_w^T [X,K], wa [R,H,K,1] -- _compact_tables)
        Wt, loop_wt, wa = ctx.forms
        g, nd, slope, halo, runs, has_loop, has_bias = ctx.g, ctx.nd, ctx.slope, ctx.halo, ctx.runs, ctx.has_loop, ctx.has_bias
        N, Kd = x.shape
        R, H, _, D = W.shape
        X = H * D
        ss, d_row, d_col = _unique_lists(g)
        rp_row, rows_node = ss["rel_ptrs_row"], ss["node_indices_row"]
        # every edge points at one of the first nd nodes (blocks, partitions: checked once per graph)?  then the
        # per-destination tensors of the backward are their first nd rows
        dst_prefix = _destinations_below(g.get_separate_coo_original()["col_indices"], nd)
        assert halo is None or dst_prefix, "a partition's edges point at owned nodes"
        # (exactly one of the three routes of the docstring; the last two add to grad_x per relation.  The bf16 node's was resolved
        #  when the call was routed -- from the same cached fact, by the same function)
        route = rgat_route.with_backward(ctx.route, lambda: dst_prefix)
        assert route.run_sums == (runs is not None) and route.halo == (halo is not None), "the forward ran another route than ctx.route"
        mulfirst, bf16 = route.mulfirst, x.dtype == th.bfloat16
        node_major, generic, per_relation_halo = (route.backward == name for name in ("node_major", "generic", "per_relation"))
        # (the weight gradient of attn_l from the edge pass when the forward left run sums: csrc/gat_compact.hip ga_block_reduce;
        #  grad_el_c then has no reader left -- its other consumer, the gradient through el, is folded into grad_feat_c -- and is
        #  not written at all)
        attn_in_pass = route.attn_in_pass
        # (the self-loop product names each of the nd output rows once: the column sums of its gradout rows ARE the bias gradient,
        #  from the weight-gradient launch that streams grad_h anyway instead of a pass of its own inside the gather op: 0.088 ms on
        #  ogbn-mag)
        # (offs = [0, nd] by construction in forward())
        # (bf16 rows: the bf16 weight-gradient entry has no column-sum form; the edge pass sums the bf16 rows on its side stream)
        bias_in_dw = not generic and has_bias and has_loop and not bf16
        main, side = th.cuda.current_stream(x.device), _side_stream(x.device) if OVERLAP and not generic else None
        if generic:
            grad_x, grad_loop, go = _per_relation_front(x, loop_w if has_loop else None, offs, grad_h, nd, H, dst_prefix)
        else:
            go = grad_h.view(nd, H, D)
            grad_loop = th.empty_like(loop_w) if has_loop else None
        ndp = go.shape[0]
        g_featc, g_erc = th.empty(featc.shape, dtype=W.dtype, device=x.device), th.empty_like(erc)  # overwritten
        # (on a partition the edge pass is handed a grad_el_c it need not write: an argument of the launch, left as it was)
        g_elc = None if attn_in_pass and halo is None else th.empty_like(elc)
        grad_bias = th.empty(X, dtype=W.dtype, device=x.device) if has_bias else None

        def loop_weight_gradient():
            if bf16:
                _k.rows_matmul_backward_dw_bf16(offs, None, x[:nd], grad_h, grad_loop.view(1, 1, Kd, X), accumulate=False)
                return
            _k.rows_matmul_backward_dw(offs, None, x[:nd], grad_h, grad_loop.view(1, 1, Kd, X), accumulate=False,
                                       colsum=grad_bias if bias_in_dw else None)
        # Everything the side stream writes is allocated before the fork (side.wait_stream(main)) that precedes the write, for the
        # reason _side_stream gives.  There are two forks: this one, in front of the self-loop's launch, which writes grad_loop and
        # grad_bias alone (allocated above); and the one in front of weight_gradients() on the node-major routes, which writes
        # grad_attn_l, grad_W (with grad_W_kx, its [R,K,X] form on the bf16 route) and grad_wa (allocated between the two).  Nothing else
        # is written from the side stream.
        if side is not None and has_loop:
            # the self-loop weight gradient needs x and grad_h only: an HBM-bound stream of rows beside the gather passes below
            # (at the start of the backward: beside the node-major pass instead it stretched the two short per-destination
            #  passes, profiles/r04/default_timeline.txt: 3.97 -> 4.02 ms)
            side.wait_stream(main)
            with th.cuda.stream(side):
                loop_weight_gradient()
        if per_relation_halo:  # the self-loop's rows of grad_x first, plain stores
            grad_x = th.empty_like(x)
            grad_x[nd:].zero_()  # halo rows: only the projection's input gradient adds to them
            _k.rows_matmul_backward_dx(offs, None, loop_wt.view(1, 1, X, Kd), grad_h, grad_x[:nd], atomic=False)
        grad_attn_l = th.empty_like(attn_l)  # (written by the edge pass on this stream, or after the second fork)
        # the bias gradient (column sums of grad_h) from the pass that reads every gradout row anyway, unless bias_in_dw
        # (the sum of grad_attn_l's partial rows is left to the side stream where the second fork follows: the node-major pass, which
        #  does not read it, starts where the edge pass ends.  ``attn_finish`` holds the workspace with those rows: it stays referenced
        #  until this function returns, i.e. past main.wait_stream(side), so no later allocation is handed its block -- _side_stream)
        attn_finish = (_k.rgat_backward_compact_bf16 if bf16 else _k.rgat_backward_compact)(
            ctx.grp, featc, elc, erc, sm[:ndp], ret[:ndp], go, g_featc, g_elc, g_erc, slope, fold_attn_l=attn_l, row_rel_ptrs=rp_row,
            grad_bias=None if bias_in_dw else grad_bias, bias_rows=nd, runs=runs, drow_nodes=ss["node_indices_col"],
            grad_attn_l=grad_attn_l if attn_in_pass else None, finish_attn_grad=not (attn_in_pass and node_major and side is not None))
        # what the launches below write: "=" outputs are allocated, "+=" outputs zero-filled
        if node_major:
            grad_x = th.empty_like(x)
        grad_W = th.zeros_like(W) if generic else th.empty_like(W)
        if mulfirst:
            grad_wa = (th.empty if node_major else th.zeros)((R, H, Kd, 1), dtype=W.dtype, device=x.device)
        # (bf16 rows: the bf16 weight-gradient entry writes [R,K,X]; the layer's [R,H,K,D] is a transposing copy of R K X floats)
        grad_W_kx = th.empty((R, 1, Kd, X), dtype=W.dtype, device=x.device) if bf16 else None

        def weight_gradients():
            # per product (four launches; each reads its own rows of x / feat_c -- a node-major pass that reads x once was
            # measured in five forms and lost: it multiplies zero rows wherever a node has no row in a relation, exp/node_dw.hip.txt)
            if not attn_in_pass:
                _k.matmul_no_scatter_gather_backward(rp_row, attn_l.unsqueeze(2), featc, g_elc, None, grad_attn_l.unsqueeze(-1),
                                                     accumulate=False)
            if generic:  # (the other three come with the input gradients below)
                return
            if has_loop and side is None:
                loop_weight_gradient()
            if bf16:
                _k.rows_matmul_backward_dw_bf16(rp_row, rows_node, x, g_featc.view(-1, X), grad_W_kx, accumulate=False)
                grad_W.copy_(grad_W_kx.view(R, Kd, H, D).transpose(1, 2))
                _k.rows_dot1h_backward_dw_bf16(ss["rel_ptrs_col"], ss["node_indices_col"], x, g_erc, grad_wa.view(R, H, Kd), False)
                return
            _k.rows_matmul_backward_dw(rp_row, rows_node, x, g_featc.view(-1, X), grad_W, accumulate=False)
            if node_major:  # the er side's weight gradient alone (its input gradient is a term of the node pass)
                _k.matmul_backward(d_col, 1, wa.view(R, H, 1, Kd), x, g_erc.view(-1, H, 1), None, grad_wa, True, accumulate=False)

        if node_major:
            row_map = _k.node_row_map(rp_row, rows_node, N)
            dst_map = _k.node_row_map(ss["rel_ptrs_col"], ss["node_indices_col"], N)
            # (on a block or a partition only the first nd nodes carry the self-loop term: they stay in front, so that term's
            #  tiles are whole too)
            order = _k.node_order_by_presence(row_map, dst_map, split=nd if nd < N else None)

            def input_gradient(begin, end):
                (_k.rgat_node_backward_dx_bf16 if bf16 else _k.rgat_node_backward_dx)(
                    begin, end, nd, grad_h if has_loop else None, loop_wt, g_featc.view(-1, X), Wt, row_map, g_erc, wa.view(R, H, Kd),
                    dst_map, grad_x, node_order=order)
            if halo is not None:
                input_gradient(nd, N)
                halo.start_return(grad_x)
            if side is not None:
                # the weight gradients (HBM-bound streams of rows) on the side stream while the node-major pass (matrix-core-bound)
                # runs on this one; both read g_featc / g_erc / grad_h, neither writes what the other reads
                # (the second fork: grad_W / grad_wa / grad_attn_l are allocated above it)
                side.wait_stream(main)
                with th.cuda.stream(side):
                    if attn_finish is not None:
                        _k.rgat_attn_grad_finish(attn_finish)
                    weight_gradients()
            input_gradient(0, N if halo is None else nd)
            if side is None:
                weight_gradients()
        else:
            if halo is not None:
                _k.rows_matmul_backward_dx(rp_row, rows_node, Wt, g_featc.view(-1, X), grad_x, atomic=2)  # rows of a relation: distinct nodes
                halo.start_return(grad_x)
            weight_gradients()
            if generic:
                _k.matmul_backward(d_row, 1, Wt, x, g_featc, grad_x, grad_W, True, accumulate=True, distinct_rows=True)
            if mulfirst:
                # the er side's weight gradient and its input gradient (destination rows: owned rows only on a partition)
                _k.matmul_backward(d_col, 1, wa.view(R, H, 1, Kd), x, g_erc.view(-1, H, 1), grad_x, grad_wa, True, accumulate=True,
                                   distinct_rows=True)
            else:  # literal er: through the destination-side projection table
                g_featd, grad_attn_r = th.empty_like(featd[0]), th.empty_like(attn_r)
                _k.matmul_no_scatter_gather_backward(ss["rel_ptrs_col"], attn_r.unsqueeze(2), featd[0], g_erc, g_featd,
                                                     grad_attn_r.unsqueeze(-1), accumulate=False)
                _k.matmul_backward(d_col, 1, Wt, x, g_featd, grad_x, grad_W, True, accumulate=True, distinct_rows=True)
        if side is not None:
            main.wait_stream(side)
        if mulfirst:
            grad_attn_r = _unfold_weight_gradient(grad_wa, W, attn_r, grad_W)
        if halo is not None:
            grad_x = halo.finish_return(grad_x[:nd])
        return _gradients(grad_x, grad_W, grad_attn_l, grad_attn_r, grad_loop, grad_bias)


def _attention_rows(g, ss, direct, grp, elc, erc, slope, N):
    """attn [E,H] in edge-id order from the tables an evaluation forward holds (csrc/gat_attention.hip): a pass over the ids, el_c
    and er_c alone, enqueued after the aggregation."""
    s, _, _ = _lists(g)
    rp, row, col, eids = s["rel_ptrs"], s["row_indices"], s["col_indices"], s["eids"]
    srow, drow = _edge_rows(g, ss, direct, rp, row, col, eids)
    return _k.rgat_attention_compact(grp, elc, erc, slope, col, srow, drow, None if _eids_are_positions(eids) else eids, N)


def _forward_only(g, direct, mulfirst, slope, num_dst, x, W, attn_l, attn_r, loop_w, bias, attn_out=None):
    """RgatLayerFunction.forward on the distinct-row dataflow when no backward can follow: a plain function (no autograd node,
    nothing saved), the same projections and the same self-loop rows, and an aggregation that writes the layer output alone
    (csrc/gat_compact.hip: the _fwd kernels) -- no lse [N,H], no ret [N,H,D], no run sums [S_col,H,D].  Every output row is bit
    for bit the training forward's.  ``attn_out`` (a list): the attention weights [E,H] are appended to it."""
    x, W, attn_l, attn_r, loop_w, nd, offs = _prologue(x, W, attn_l, attn_r, loop_w, num_dst)
    R, H, _, D = W.shape
    ss, h, saved, grp, _, _ = _compact_tables(g, direct, mulfirst, None, nd, offs, x, W, attn_l, attn_r, loop_w, bias)
    featc, elc, erc = saved[:3]
    fused = h is not None
    if not fused:  # no self-loop rows to add into (no self-loop, or widths its fused launch does not take): zeros, the tail below
        h = x.new_zeros((nd, H * D))
    _k.rgat_aggregate_compact_forward(grp, featc, elc, erc, h, slope, R, attn_l=attn_l, feat_rel_ptrs=ss["rel_ptrs_row"])
    if attn_out is not None:
        attn_out.append(_attention_rows(g, ss, direct, grp, elc, erc, slope, x.shape[0]))
    if fused:
        return h
    # (the training forward clones its view of ret when there is nothing to add; h is already a buffer of its own)
    rows = _loop_and_bias_rows(h, x, nd, offs, loop_w, bias)
    return h if rows is None else rows


def _bf16_tables(g, direct, num_dst, x, W, attn_l, attn_r, loop_w, bias, training):
    """The bf16 forward in front of its aggregation, common to _forward_only_bf16 and RgatLayerBf16Function.forward: feat_c (bf16) on
    the unique (relation, source) rows, er_c from the folded weight, the self-loop + bias rows h (bf16) the aggregation adds into,
    and el_c -- a row-dot pass over the rounded feat_c -- where the walk gathers it or a backward follows (``training``; else None).
    Returns (operands, nd, ss, featc, elc, erc, h, grp, offs, forms); operands = the contiguous (x, W, attn_l, attn_r, loop_w),
    forms = the parameter forms of _compact_tables (all fp32) when ``training``, else None."""
    # (the cached [0, nd] list and a copy of the self-loop weight are made here, under the main stream)
    x, W, attn_l, attn_r, loop_w, nd, offs = _prologue(x, W, attn_l, attn_r, loop_w, num_dst)
    s, _, _ = _lists(g)
    rp, row, col, eids = s["rel_ptrs"], s["row_indices"], s["col_indices"], s["eids"]
    N = x.shape[0]
    R, H, Kd, D = W.shape
    X = H * D
    dev = x.device
    ss = g.get_separate_unique_node_indices_single_sided()
    # (everything the side stream writes is allocated before the fork: _side_stream)
    featc = th.empty((ss["node_indices_row"].numel(), H, D), dtype=th.bfloat16, device=dev)
    erc = th.empty((ss["node_indices_col"].numel(), H), dtype=th.float32, device=dev)
    elc = None if _k.rgat_el_from_row(H, D, R) and not training else th.empty((featc.shape[0], H), dtype=th.float32, device=dev)
    bias_c = None if bias is None else bias.contiguous()
    if loop_w is not None:
        h = th.empty((nd, X), dtype=th.bfloat16, device=dev)
    elif bias_c is not None:  # no self-loop: the rows the aggregation adds into hold the (rounded) bias alone
        h = bias_c.to(th.bfloat16).expand(nd, X).contiguous()
    else:
        h = th.zeros((nd, X), dtype=th.bfloat16, device=dev)
    wa = _folded_weight(W, attn_r)  # (fp32; in front of the fork, as in _compact_tables)
    main = th.cuda.current_stream(dev)
    side = _side_stream(dev) if OVERLAP else None
    if side is not None:
        side.wait_stream(main)
    with th.cuda.stream(side if side is not None else main):  # er_c and the self-loop: HBM-bound streams of rows beside the projection
        _k.rows_dot1h_bf16(ss["rel_ptrs_col"], ss["node_indices_col"], wa.view(R, H, Kd), x, erc)
        if loop_w is not None:
            _k.rows_linear_bias_bf16(offs, x[:nd], loop_w, bias_c, out=h)
    _k.rows_matmul_heads_bf16(ss["rel_ptrs_row"], ss["node_indices_row"], W, x, featc)
    if elc is not None:
        _k.rgat_el_rows_bf16(ss["rel_ptrs_row"], featc, attn_l, elc)
    # (the transposes of the parameters, for the backward: one launch on the main stream, which has slack here -- _compact_tables)
    forms = _k.rgat_transpose_weights(W, loop_w) + (wa,) if training else None
    if side is not None:
        main.wait_stream(side)
    srow, drow = _edge_rows(g, ss, direct, rp, row, col, eids)
    grp = _k.rgat_compact_groupings(col, srow, drow, N, featc.shape[0], erc.shape[0], rel_ptrs=rp,
                                    drow_nodes=ss["node_indices_col"], drow_rel_ptrs=ss["rel_ptrs_col"])
    return (x, W, attn_l, attn_r, loop_w), nd, ss, featc, elc, erc, h, grp, offs, forms


def _forward_only_bf16(g, direct, slope, num_dst, x, W, attn_l, attn_r, loop_w, bias, attn_out=None):
    """_forward_only for a bf16 input (the module docstring has the precision contract): feat_c [S_row,H,D] and h [nd,X] are bf16
    rows, no fp32 copy of x, feat_c or h is made, and the aggregation rounds h once more where it adds a destination's row in place.
    The same launches as the fp32 path except that el_c, where the walk gathers it, is a row-dot pass over the rounded feat_c
    instead of the projection's epilogue.  ``attn_out`` (a list): the attention weights [E,H] (fp32) are appended to it; where the
    walk formed el from the row it gathered, el_c is made for them by the same row-dot pass, so they are the softmax the output used."""
    (x, W, attn_l, attn_r, loop_w), nd, ss, featc, elc, erc, h, grp, _, _ = _bf16_tables(g, direct, num_dst, x, W, attn_l, attn_r, loop_w,
                                                                                         bias, False)
    R, H, _, D = W.shape
    _k.rgat_aggregate_compact_forward_bf16(grp, featc, elc, erc, h, slope, R, attn_l=attn_l, feat_rel_ptrs=ss["rel_ptrs_row"])
    if attn_out is not None:
        if elc is None:
            elc = th.empty((featc.shape[0], H), dtype=th.float32, device=x.device)
            _k.rgat_el_rows_bf16(ss["rel_ptrs_row"], featc, attn_l, elc)
        attn_out.append(_attention_rows(g, ss, direct, grp, elc, erc, slope, x.shape[0]))
    return h


@_consistent_plan
class RgatLayerBf16Function(th.autograd.Function):
    """The layer's training step on bf16 rows (the module docstring): _forward_only_bf16's launches with the training aggregation,
    which also leaves lse, ret and the run sums (fp32), and el_c always (the edge pass of the backward reads it); the backward is
    RgatLayerFunction._backward_distinct_rows on its node-major route.  Saved: x and feat_c as bf16."""

    @staticmethod
    def forward(ctx, g, route, slope, num_dst, x, W, attn_l, attn_r, loop_w, bias):
        (x, W, attn_l, attn_r, loop_w), nd, ss, featc, elc, erc, h, grp, offs, ctx.forms = _bf16_tables(g, route.direct, num_dst, x, W, attn_l,
                                                                                                        attn_r, loop_w, bias, True)
        N = x.shape[0]
        R, H, _, D = W.shape
        sm = th.empty((N, H), dtype=th.float32, device=x.device)
        ret = th.empty((N, H, D), dtype=th.float32, device=x.device)
        ctx.runs = _k.rgat_aggregate_compact_bf16(grp, featc, elc, erc, sm, ret, slope, h, R, attn_l=attn_l, feat_rel_ptrs=ss["rel_ptrs_row"])
        ctx.grp, ctx.halo = grp, None
        ctx.g, ctx.route, ctx.slope, ctx.nd = g, route, slope, nd
        ctx.has_loop, ctx.has_bias = loop_w is not None, bias is not None
        none = W.new_empty(0)
        ctx.save_for_backward(x, W, attn_l, attn_r, loop_w if loop_w is not None else none, offs if offs is not None else none, sm, none,
                              ret, featc, elc, erc)
        return h

    @staticmethod
    def backward(ctx, grad_h):
        grads = RgatLayerFunction._backward_distinct_rows(ctx, grad_h.contiguous())
        return (None, None, None, None) + grads[5:]  # (g, route, slope, num_dst; then x and the parameters)


def attention_composition(g, x, W, attn_l, attn_r, slope):
    """The attention weights [E,H] (float32, edge-id order) of the layer as a plain torch composition under no_grad, in fp32 whatever
    the input type: per-relation projections of the distinct source / destination nodes, exponentials relative to the destination's
    maximum summed with index_add, a divide.  For every call the evaluation kernels do not serve (a gradient is required, halo,
    per-edge dataflow, op by op, the reference's op sequence, CPU tensors, other shapes): correct, not fast -- R small GEMMs and
    several [E,H] temporaries."""
    with th.no_grad():
        s = g.get_separate_coo_original()
        rp, row, col, eids = s["rel_ptrs"], s["row_indices"], s["col_indices"], s["eids"]
        x, W, attn_l, attn_r = x.detach().float(), W.detach().float(), attn_l.detach().float(), attn_r.detach().float()
        R, H, Kd, D = W.shape
        E, N = row.numel(), x.shape[0]
        z = x.new_empty((E, H))
        for r, (a, b) in enumerate(zip(rp[:-1].tolist(), rp[1:].tolist())):
            if a == b:
                continue
            Wr = W[r].permute(1, 0, 2).reshape(Kd, H * D)
            src, isrc = th.unique(row[a:b], return_inverse=True)
            dst, idst = th.unique(col[a:b], return_inverse=True)
            el = ((x[src] @ Wr).view(-1, H, D) * attn_l[r]).sum(-1)
            er = ((x[dst] @ Wr).view(-1, H, D) * attn_r[r]).sum(-1)
            z[a:b] = el[isrc] + er[idst]
        sc = th.where(z > 0, z, z * slope)
        idx = col.unsqueeze(-1).expand(-1, H)
        m = th.full((N, H), -float("inf"), dtype=sc.dtype, device=sc.device).scatter_reduce(0, idx, sc, "amax")
        w = th.exp(sc - m[col])
        den = th.zeros((N, H), dtype=sc.dtype, device=sc.device).index_add_(0, col, w)
        attn = th.empty_like(w)
        attn[eids] = w / den[col]
        return attn


def rgat_layer_fused(route, g, x, W, attn_l, attn_r, loop_w, bias, slope, num_dst=None, halo=None, attn_out=None):
    """Run ``route`` (rgat_route.decide's answer for this call; the operands at its widths).  ``attn_out`` (a list, optional): on the
    evaluation paths the attention weights [E,H] are appended to it (_forward_only / _forward_only_bf16); the autograd nodes leave
    it empty and the caller composes them (attention_composition)."""
    if route.compact and not _has_single_sided_lists(g):
        g.generate_separate_unique_node_indices_single_sided_for_each_etype()
    if route.path == "node":
        return RgatLayerFunction.apply(g, route, float(slope), num_dst, halo, x, W, attn_l, attn_r, loop_w, bias)
    if route.path == "train_bf16":
        return RgatLayerBf16Function.apply(g, route, float(slope), num_dst, x, W, attn_l, attn_r, loop_w, bias)
    with th.no_grad():
        if route.path == "eval":
            return _forward_only(g, route.direct, route.mulfirst, float(slope), num_dst, x, W, attn_l, attn_r, loop_w, bias, attn_out)
        if route.path == "eval_bf16":
            return _forward_only_bf16(g, route.direct, float(slope), num_dst, x, W, attn_l, attn_r, loop_w, bias, attn_out)
    raise _k._lib.HetError(f"rgat_layer_fused: no kernels behind the path {route.path!r}")
