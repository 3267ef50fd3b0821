"""HGT attention + aggregation (HGT/models.py:120-262) as ONE autograd node on the distinct (relation, source) rows.

The op-by-op composition in het_amd/layers.py follows the reference's model code: typed K / Q / V projections of every
node, relation_att applied per (relation, destination) row, an inner product per edge, the edge softmax and the message
product fused with the aggregation -- with [E,H] / [E,H,dk] tensors between them.  Here, for graphs whose relations are
canonical edge types (one source node type each -- what the reference's HGT requires too, HGT/models.py:31-52):

  w_kv[r] = [ K_st(r) . att'[r] . pri[r] / sqrt(dk)  |  V_st(r) . msg[r] ]     [in, 2*H*dk], built per step from the parameters
                                                       with torch ops (autograd carries the gradient back to k_linears,
                                                       relation_att, relation_pri, v_linears, relation_msg) -- the
                                                       reference's --multiply_among_weights_first_flag idea
                                                       (HGT/models.py:124-151) applied to the source side
  kv_c    = h[src of row] . w_kv[r of row]            one segment GEMM over the S_row distinct (relation, source) rows
  q       = typed projection of the nodes
  new_h   = het_hgt_aggregate_compact(kv_c, q)        softmax + aggregation, csrc/hgt_compact.hip

att' = relation_att for --hgt_fused_attn_score_flag (s = <k . att, q>), its transpose otherwise (s = <q . att, k>).
Same function of the parameters as the composition (associativity of the matrix products): tests/ check both against
oracle/layers.py::hgt_layer.  HET_HGT_FUSED=0 keeps the composition.

Which calls run here, at which widths, with which output projection and which form of the backward is decided once per call, by
hgt_route.decide: the table of its module docstring has every path with its conditions.  hgt_layer_fused runs the record it is
given, and HgtAttentionFunction keeps it on its context for the backward.
"""
import os

import torch as th

from ..plan import consistent as _consistent_plan

from .. import kernels as _k
from ..kernels import K
from .rgat_fused_layer import OVERLAP, _edge_rows, _has_single_sided_lists, _side_stream
from .rgnn_layers_and_funcs import rgnn_relational_matmul_no_scatter_gather_list as B_matmul_no_scatter_gather

FUSED = os.environ.get("HET_HGT_FUSED", "1") != "0"


def _node_dx_plan(G, rp_row, rows_node, offs, K_in, X, dst):
    """Per graph, cached on it: what the node-major input gradient needs -- [R,N] int32 row maps of the (relation, source) list,
    the rank of every node in the list of destinations with in-edges (``dst`` = (dst_nodes, run_ptrs): the compact form), the nodes
    sorted by (node type, which sources they have rows in) so that 32-node tiles are homogeneous, and per node type its position
    range + relations.
    (Whether the pass serves the graph and the shapes: ``dx`` of hgt_route.decide.)"""
    key = ("hgt_node_dx", K_in, X, dst is not None)
    plan = G._plans.get(key)
    if plan is None:
        with _k._plan.building():  # (kept on the graph: normal tensors whatever the caller's mode)
            plan = G._plans[key] = _build_node_dx_plan(G, rp_row, rows_node, offs, dst)
    return plan


def _build_node_dx_plan(G, rp_row, rows_node, offs, dst):
    st_l, offs_l = G.get_rel_node_types()[0].tolist(), offs.tolist()
    T, R, N = len(offs_l) - 1, len(st_l), offs_l[-1]
    row_map = _k.node_row_map(rp_row, rows_node, N)
    dev = row_map.device
    dst_rank, has_dst = None, [True] * T
    if dst is not None:
        dst_nodes, run_ptrs = dst
        dst_rank = th.full((N,), -1, dtype=th.int32, device=dev)
        dst_rank[dst_nodes] = th.arange(dst_nodes.numel(), dtype=th.int32, device=dev)
        has_dst = (run_ptrs[1:] > run_ptrs[:-1]).tolist()
    w = (1 << th.arange(R, device=dev, dtype=th.int64)).view(R, 1)
    mask = ((row_map >= 0).to(th.int64) * w).sum(0)
    if dst_rank is not None:
        mask = mask | ((dst_rank >= 0).to(th.int64) << R)
    typ = th.searchsorted(offs[1:].contiguous().to(dev), th.arange(N, device=dev), right=True)
    order = th.argsort(mask | (typ << (R + 1)), stable=True).to(th.int32).contiguous()
    return dict(row_map=row_map, dst_rank=dst_rank, order=order, offs=offs_l, has_dst=has_dst,
                rels_of=[[r for r in range(R) if st_l[r] == t] for t in range(T)])


def graph_facts(G, offs):
    """What hgt_route.decide is told about the graph: the ``edges``, ``lists``, ``lists_present`` and ``typed_runs`` of its
    Facts, and the three facts that read the graph's arrays, as callables for decide to ask where they matter."""
    graph, present = hasattr(G, "graph_data"), _has_single_sided_lists(G)
    facts = dict(edges=graph and G.get_num_edges() > 0, lists_present=present,
                 lists=present or hasattr(G, "generate_separate_unique_node_indices_single_sided_for_each_etype"),
                 typed_runs=graph and G.graph_data["original"].get("node_segment_types") is not None)

    def canonical():
        try:
            return bool(G.get_rel_node_types())
        except ValueError:  # a relation mixes node types: no single K / V projection per relation to fold
            return False
    # (read back to the host once per graph)
    rels_per_type = lambda: _k._derived_get("hgt_rels_per_type", (G.get_rel_node_types()[0], offs),
                                            lambda: th.bincount(G.get_rel_node_types()[0], minlength=offs.numel() - 1).tolist())
    return facts, canonical, lambda: _k.destination_lists(G.get_separate_coo_original()["col_indices"], offs)[0].numel(), rels_per_type


def _head_groups(num_heads: int, d_pad: int):
    """Number of head groups the attention runs in: 1 when the row kernels take all heads' rows at once (up to 128 floats per
    row), else the smallest split into equal groups they do take -- heads are independent up to the output projection, so 8
    heads of 32 floats (out = 256) run as two passes over 4 heads each (ogbn-mag: 53 -> 27 ms per step; the op-by-op composition
    before).  None: no split fits (one head wider than 128 floats)."""
    for groups in (1, 2, 4, 8):
        if num_heads % groups == 0 and _k.hgt_compact_shape_ok(num_heads // groups, d_pad):
            return groups
    return None


def _padded_head(d_k: int) -> int:
    """Head width the row kernels run with: a power of two >= 8.  Narrower / odd heads (the 8 classes of the reference CLI's
    last layer split over 4 heads: d_k = 2) are zero-padded -- zero columns in the folded weights and in the typed projection
    of q add nothing to a score, and the padded components of the aggregated messages are dropped."""
    return max(8, 1 << max(0, int(d_k) - 1).bit_length())


def _pad_heads(w, num_heads, d_k, d_pad, parts=1):
    """[..., parts * H * d_k] -> [..., parts * H * d_pad] with zero columns after every head's d_k."""
    if d_pad == d_k:
        return w
    lead = w.shape[:-1]
    return th.nn.functional.pad(w.reshape(*lead, parts * num_heads, d_k), (0, d_pad - d_k)).reshape(*lead, parts * num_heads * d_pad)


FOLD_KERNEL = os.environ.get("HET_HGT_FOLD_KERNEL", "1") == "1"  # A/B: the torch composition below instead of the two HIP launches


class _FoldSourceWeights(th.autograd.Function):
    """fold_source_weights as one HIP launch and its backward as two (csrc/hgt_fold.hip): written with torch ops the folding is ~14
    launches of a few microseconds each per step and ~24 more in autograd's backward -- 0.3 ms of HGT's 6.4 ms step on ogbn-mag."""

    @staticmethod
    def forward(ctx, k_lin, v_lin, rel_att, rel_msg, rel_pri, src_type, fused_attn):
        args = tuple(t.contiguous() for t in (k_lin, v_lin, rel_att, rel_msg, rel_pri))
        ctx.save_for_backward(*args, src_type)
        ctx.transpose = not fused_attn
        return _k.hgt_fold_source_weights(*args, src_type, ctx.transpose)

    @staticmethod
    def backward(ctx, grad_w):
        *args, src_type = ctx.saved_tensors
        return (*_k.hgt_fold_source_weights_backward(grad_w.contiguous(), *args, src_type, ctx.transpose), None, None)


def fold_source_weights(k_lin, v_lin, rel_att, rel_msg, rel_pri, src_type, num_heads, fused_attn):
    """w_kv [R,1,in,2*H*dk] (module docstring).  k_lin / v_lin [T,1,in,H*dk]; rel_att / rel_msg [R,H,dk,dk]; rel_pri [R,H]."""
    if (FOLD_KERNEL and k_lin.is_cuda and k_lin.dtype == th.float32 and k_lin.dim() == 4 and k_lin.shape[1] == 1
            and src_type.is_cuda and src_type.dtype == th.int64):
        return _FoldSourceWeights.apply(k_lin, v_lin, rel_att, rel_msg, rel_pri, src_type.contiguous(), fused_attn)
    R, H, dk, _ = rel_att.shape
    K_in = k_lin.shape[2]
    heads = lambda w: w.index_select(0, src_type).view(R, K_in, H, dk).permute(0, 2, 1, 3)  # [R,H,in,dk]
    att = rel_att if fused_attn else rel_att.transpose(2, 3)
    mu = (rel_pri / (dk ** 0.5)).view(R, H, 1, 1)
    wk = th.matmul(heads(k_lin), att * mu)   # [R,H,in,dk]
    wm = th.matmul(heads(v_lin), rel_msg)
    flat = lambda w: w.permute(0, 2, 1, 3).reshape(R, K_in, H * dk)
    return th.cat([flat(wk), flat(wm)], dim=2).unsqueeze(1).contiguous()


def _row_lists(rel_ptrs, rows):
    """A (relation, node) list whose rows are distinct inside every relation, as the segment GEMM entries take it."""
    return {"unique_srcs_and_dests_rel_ptrs": rel_ptrs, "unique_srcs_and_dests_node_indices": rows}


# Destinations WITHOUT in-edges receive nothing: their rows of new_h are zero, and so are their rows of the layer output
# (the typed output projection has no bias).  When they are many (on the ogbn-mag-like graph 58 % of the nodes), q, lsum,
# new_h and the output projection live on the S_dst destinations that do have in-edges: the row kernels are agnostic (their
# "node" is then the rank of the destination in the sorted list of those), the two typed projections run on S_dst rows.
COMPACT_DST_BELOW = float(os.environ.get("HET_HGT_COMPACT_DST", "0.8"))  # use the lists when S_dst < this fraction of N


@_consistent_plan
class HgtAttentionFunction(th.autograd.Function):
    @staticmethod
    def forward(ctx, G, route, num_heads, offs, h, w_kv, q_w, dst):
        """h [N,in]; w_kv [R,1,in,2X]; q_w [T,1,in,X] typed projection of the destination side (one weight per run of offs).
        dst = None: rows of the result are nodes.  dst = (dst_nodes, rank_of_edge, run_ptrs) (kernels.destination_lists, with
        ``route.compact_dst``): rows are the destinations with in-edges, in that order.  ``route``: hgt_route.decide's answer for the
        call -- a bf16 h only with ``native_bf16``, so in the shapes of the bf16 kernels; the backward reads its own route from it."""
        h, w_kv, q_w = h.contiguous(), w_kv.contiguous(), q_w.contiguous()
        N, X = h.shape[0], q_w.shape[3]
        s = G.get_separate_coo_original()
        ss = G.get_separate_unique_node_indices_single_sided()
        rp_row, rows_node = ss["rel_ptrs_row"], ss["node_indices_row"]
        S_row = rows_node.numel()
        bf16 = h.dtype == th.bfloat16  # activation rows (h, kv_c, q, out) bf16; lsum and every parameter fp32 (hgt_layer_fused)
        new = lambda *shape: th.empty(shape, dtype=h.dtype, device=h.device)
        # the destination-side projection beside the source-row one (rgat_fused_layer._side_stream: independent launches, the
        # tensors are allocated and freed under the main stream)
        main, side = th.cuda.current_stream(h.device), (_side_stream(h.device) if OVERLAP and h.is_cuda else None)
        dst_nodes, keys, run_ptrs = (None, s["col_indices"], offs) if dst is None else dst  # (the rows of q: every node, in runs of offs)
        ND = N if dst is None else dst_nodes.numel()
        q, kv_c = new(ND, X) if dst is None else new(ND, 1, X), new(S_row, 1, 2 * X)
        if side is not None:
            side.wait_stream(main)
        with th.cuda.stream(side if side is not None else main):
            if bf16:
                _k.rows_matmul_bf16(run_ptrs, dst_nodes, None, q_w, h, q.view(ND, X))
            elif dst is None:
                K.rgnn_relational_matmul_no_scatter_gather_list(offs, q_w, h, q)
            else:
                K.rgnn_relational_matmul(_row_lists(run_ptrs, dst_nodes), 1, q_w, h, q, True)
        q = q.view(ND, X)
        if bf16:
            _k.rows_matmul_bf16(rp_row, rows_node, None, w_kv, h, kv_c.view(S_row, 2 * X))
        else:
            K.rgnn_relational_matmul(_row_lists(rp_row, rows_node), 1, w_kv, h, kv_c, True)
        if side is not None:
            main.wait_stream(side)
        srow, _ = _edge_rows(G, ss, True, s["rel_ptrs"], s["row_indices"], s["col_indices"], s["eids"])
        grp = _k.hgt_compact_groupings(keys, srow, ND, S_row)
        lsum, out = th.empty((ND, num_heads), dtype=th.float32, device=h.device), new(ND, X)
        (_k.hgt_aggregate_compact_bf16 if bf16 else _k.hgt_aggregate_compact)(grp, kv_c, q, lsum, out)
        ctx.G, ctx.route, ctx.grp = G, route, grp
        ctx.save_for_backward(h, w_kv, q_w, offs, q, kv_c, lsum, out, *(() if dst is None else (dst[0], dst[2])))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        h, w_kv, q_w, offs, q, kv_c, lsum, out, *lists = ctx.saved_tensors
        # sums over edges, hub rows met by float atomics, streamed once into the fp32 parameter gradients: fp32 for either row type
        g_kv, g_q = th.empty_like(kv_c, dtype=th.float32), th.empty_like(q, dtype=th.float32)
        bwd = _k.hgt_backward_compact_bf16 if h.dtype == th.bfloat16 else _k.hgt_backward_compact
        bwd(ctx.grp, kv_c, q, lsum, out, grad_out.contiguous(), g_kv, g_q)
        return (None,) * 4 + _DenseBackward(ctx.route, ctx.G, h, w_kv, q_w, offs, lists, g_kv, g_q).run() + (None,)


class _DenseBackward:
    """The dense half of HgtAttentionFunction.backward: from g_kv [S_row,1,2X] and g_q [ND,X], the gradients of h, w_kv and q_w on
    the route of the call (hgt_route.decide: ``dx``, ``split_kv``, ``split_q``, ``compact_dst``).
    The two weight gradients (HBM-bound streams of rows; ``dw`` has their one launch) follow one rule in every form of the input
    gradient.  With a side stream (HET_RGAT_OVERLAP; rgat_fused_layer._side_stream) they run there, beside the input-gradient chain:
    w_kv's right after the first fork (where the route has ``split_kv``), q's after a second fork that follows the allocation of its
    buffer.  Without one, each runs on the main stream where the form places its ``dw``."""

    def __init__(self, route, G, h, w_kv, q_w, offs, lists, g_kv, g_q):
        self.route, self.G, self.h, self.w_kv, self.q_w, self.offs, self.lists, self.g_kv, self.g_q = route, G, h, w_kv, q_w, offs, lists, g_kv, g_q
        self.X = X = q_w.shape[3]
        ss = G.get_separate_unique_node_indices_single_sided()
        self.rp_row, self.rows_node = ss["rel_ptrs_row"], ss["node_indices_row"]
        # the rows of the destination-side projection: the destinations with in-edges in runs of a node type, or every node
        self.rp_q, self.rows_q = (lists[1], lists[0]) if route.compact_dst else (offs, None)
        self.g_kv2 = g_kv.view(-1, 2 * X)
        self.pending = {"kv": (self.rp_row, self.rows_node, self.g_kv2), "q": (self.rp_q, self.rows_q, g_q)}
        # one input-gradient buffer for both consumers of h
        self.qwt, self.wt = q_w.transpose(2, 3).contiguous(), w_kv.transpose(2, 3).contiguous()
        self.main, self.side = th.cuda.current_stream(h.device), (_side_stream(h.device) if OVERLAP and h.is_cuda else None)

    def dw(self, early=False, **grad_w):
        """Launch the weight gradients (which=buffer) that are not launched yet: on the side stream, forked here, or without one on
        the main stream -- unless ``early``: a place where only the side stream launches."""
        todo = [which for which in grad_w if which in self.pending and not (early and self.side is None)]
        if todo and self.side is not None:
            # A fork per place: grad_qw (and, on a graph seen for the first time, the node-major plan's temporaries) are allocated AFTER
            # the first fork, so the allocator may have handed out blocks whose previous main-stream use was enqueued after that fork
            # (the kernels that build the plan), and the side stream would write grad_qw while they still run -- seen once in ~40 cold
            # runs as rows of grad_h missing (the node order came out corrupted).  A fork is free when nothing is pending.
            self.side.wait_stream(self.main)
        rows_dw = _k.rows_matmul_backward_dw_bf16 if self.h.dtype == th.bfloat16 else _k.rows_matmul_backward_dw
        with th.cuda.stream(self.main if self.side is None else self.side):
            for which in todo:
                rel_ptrs, rows, g = self.pending.pop(which)
                rows_dw(rel_ptrs, rows, self.h, g, grad_w[which], accumulate=False)

    def run(self):
        grad_wkv = th.empty_like(self.w_kv) if self.route.split_kv else None
        if self.route.split_kv:
            self.dw(early=True, kv=grad_wkv)
        grad_h, grad_wkv, grad_qw = getattr(self, self.route.dx)(grad_wkv)
        if self.side is not None:
            self.main.wait_stream(self.side)  # (a wait for a stream without new work is free)
        return grad_h.to(self.h.dtype), grad_wkv, grad_qw

    def node_major(self, grad_wkv):
        """Every consumer of h adds its term in ONE pass over the nodes (csrc/node_sum.hip) -- instead of one read-modify-write
        launch per relation on the 2X-wide source rows + the destination-side projection's own pass (the round-3 form): the
        destination-side projection's gradient rows (g_q . Q_t^T) and, per relation the node is a source of, the two halves of its
        [k' | m] gradient row."""
        h, X = self.h, self.X
        nplan = _node_dx_plan(self.G, self.rp_row, self.rows_node, self.offs, h.shape[1], X, self.lists or None)
        grad_h, grad_qw = th.empty_like(h), th.empty_like(self.q_w)  # (allocated under the main stream)
        self.dw(kv=grad_wkv, q=grad_qw)  # the other two weight gradients beside the node pass
        node_sum = _k.node_rows_matmul_sum_bf16 if h.dtype == th.bfloat16 else _k.node_rows_matmul_sum
        wt2 = self.wt.view(-1, 2 * X, h.shape[1])
        for t, rels in enumerate(nplan["rels_of"]):
            a, b = nplan["offs"][t], nplan["offs"][t + 1]
            srcs = []
            if nplan["has_dst"][t]:
                srcs.append((self.g_q, 0, nplan["dst_rank"], self.qwt[t, 0]))
            for r in rels:
                srcs.append((self.g_kv2, 0, nplan["row_map"][r], wt2[r, :X]))
                srcs.append((self.g_kv2, X, nplan["row_map"][r], wt2[r, X:]))
            if not srcs:
                grad_h[a:b].zero_()  # (a node type that neither sends nor receives: its rows of the gradient are zero)
            elif b > a:
                node_sum(a, b, srcs, grad_h, nplan["order"])
        return grad_h, grad_wkv, grad_qw

    def fp32_buffer(self, grad_wkv):
        """bf16 rows and more relations per node type than the node-major pass keeps in LDS: the per-relation launches add a node's
        terms in an fp32 buffer, which ``run`` rounds once (the only fp32 [N, in] tensor of the bf16 step; h itself is never widened)."""
        grad_h32 = (th.zeros if self.route.compact_dst else th.empty)(self.h.shape, dtype=th.float32, device=self.h.device)
        grad_qw = th.empty_like(self.q_w)
        self.dw(kv=grad_wkv, q=grad_qw)
        _k.rows_matmul_backward_dx(self.rp_q, self.rows_q, self.qwt, self.g_q, grad_h32, atomic=False)
        _k.rows_matmul_backward_dx(self.rp_row, self.rows_node, self.wt, self.g_kv2, grad_h32, atomic=2)
        return grad_h32, grad_wkv, grad_qw

    def per_relation(self, grad_wkv):
        """fp32 rows outside the node-major pass: the destination-side projection writes its rows of grad_h, the source-row GEMM adds
        to them relation by relation; widths outside rows_matmul_backward_split_ok take the any-shape dX + dW launch."""
        r, h = self.route, self.h
        if not r.compact_dst:  # the typed projection writes every row with plain stores
            grad_h, grad_qw = th.empty_like(h), th.empty_like(self.q_w)
            _k.matmul_no_scatter_gather_backward(self.offs, self.qwt, h, self.g_q, grad_h, grad_qw, accumulate=False)
        elif r.split_q:
            grad_h, grad_qw = th.zeros_like(h), th.empty_like(self.q_w)
            self.dw(early=True, q=grad_qw)
            _k.rows_matmul_backward_dx(self.rp_q, self.rows_q, self.qwt, self.g_q, grad_h, atomic=False)  # distinct nodes, first writer: "="
            self.dw(q=grad_qw)
        else:
            grad_h, grad_qw = th.zeros_like(h), th.zeros_like(self.q_w)
            _k.matmul_backward(_row_lists(self.rp_q, self.rows_q), 1, self.qwt, h, self.g_q.view(-1, 1, self.X), grad_h, grad_qw, True,
                               accumulate=True, distinct_rows=True)
        if r.split_kv:
            _k.rows_matmul_backward_dx(self.rp_row, self.rows_node, self.wt, self.g_kv2, grad_h, atomic=2)  # rows of a relation: distinct nodes
            self.dw(kv=grad_wkv)
        else:
            grad_wkv = th.zeros_like(self.w_kv)
            _k.matmul_backward(_row_lists(self.rp_row, self.rows_node), 1, self.wt, h, self.g_kv, grad_h, grad_wkv, True, accumulate=True,
                               distinct_rows=True)
        return grad_h, grad_wkv, grad_qw


@_consistent_plan
class RowsLinearScatter(th.autograd.Function):
    """out[rows[i], :] = x_c[i, :] . w[t(i)] for the listed rows, zero elsewhere: a typed projection of compact rows written
    straight into the dense result (and its gradient read straight from the dense gradient) -- no index_copy / index_select
    passes.  rows are distinct and sorted, ``run_ptrs`` [T+1] splits them into the runs of ``w`` [T,1,K,X]."""

    @staticmethod
    def forward(ctx, run_ptrs, rows, num_out_rows, x_c, w):
        x_c, w = x_c.contiguous(), w.contiguous()
        out = th.zeros((num_out_rows, w.shape[3]), dtype=w.dtype, device=w.device)
        # (the "transposed weight" slot of the dX entry point takes [T,1,D_in,K_out]: exactly w)
        _k.rows_matmul_backward_dx(run_ptrs, rows, w, x_c, out, atomic=False)
        ctx.save_for_backward(run_ptrs, rows, x_c, w)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        run_ptrs, rows, x_c, w = ctx.saved_tensors
        grad_out = grad_out.contiguous()
        T, _, K_in, X_out = w.shape
        g_x = th.empty((x_c.shape[0], 1, K_in), dtype=w.dtype, device=w.device)
        # g_x[i] = grad_out[rows[i]] . w[t]^T
        K.rgnn_relational_matmul(_row_lists(run_ptrs, rows), 1, w.transpose(2, 3).contiguous(), grad_out, g_x, True)
        g_wt = th.empty((T, 1, X_out, K_in), dtype=w.dtype, device=w.device)
        _k.rows_matmul_backward_dw(run_ptrs, rows, grad_out, x_c, g_wt, accumulate=False)  # SUM grad_out[rows[i]]^T (x) x_c[i]
        return None, None, None, g_x.view_as(x_c), g_wt.transpose(2, 3)


class RowsLinearBf16(th.autograd.Function):
    """The typed output projection with bf16 rows: out[rows[i], :] = x[i, :] . w[t(i)] (``rows`` None: row i), zero elsewhere.  x, out
    and their gradients bf16 (each rounded once at its kernel's store), ``w`` [T,1,K,X] and its gradient fp32; ``run_ptrs`` [T+1]
    splits the rows into the runs of ``w``."""

    @staticmethod
    def forward(ctx, run_ptrs, rows, num_out_rows, x, w):
        x, w = x.contiguous(), w.contiguous()
        alloc = th.empty if rows is None else th.zeros
        out = alloc((num_out_rows, w.shape[3]), dtype=th.bfloat16, device=x.device)
        _k.rows_matmul_bf16(run_ptrs, None, rows, w, x, out)
        ctx.save_for_backward(run_ptrs, x, w, *(() if rows is None else (rows,)))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        run_ptrs, x, w, *rows = ctx.saved_tensors
        rows = rows[0] if rows else None
        grad_out = grad_out.contiguous()
        g_x, g_w = th.empty_like(x), th.empty_like(w)
        main, side = th.cuda.current_stream(x.device), (_side_stream(x.device) if OVERLAP else None)
        if side is not None:  # (forked after the allocations above: HgtAttentionFunction.backward says why)
            side.wait_stream(main)
        with th.cuda.stream(side if side is not None else main):
            _k.rows_matmul_backward_dw_bf16(run_ptrs, None, x, grad_out, g_w, accumulate=False, g_rows=rows)
        _k.rows_matmul_bf16(run_ptrs, rows, None, w.transpose(2, 3).contiguous(), grad_out, g_x)  # g_x[i] = grad_out[rows[i]] . w[t]^T
        if side is not None:
            main.wait_stream(side)
        return None, None, None, g_x, g_w


def _typed_layer_norm_kernel_ok(y):
    """Rows the layer-norm kernels take: a contiguous fp32 or bf16 [N, X] GPU tensor of a served width whose rows are 16-byte
    (bf16: 8-byte) aligned."""
    return (y.is_cuda and y.dim() == 2 and y.dtype in (th.float32, th.bfloat16) and y.is_contiguous()
            and _k.rows_layer_norm_ok(y.shape[1]) and y.data_ptr() % (4 * y.element_size()) == 0)


@_consistent_plan
class TypedLayerNormFunction(th.autograd.Function):
    """out[v] = LayerNorm(y[v]) * gamma[t(v)] + beta[t(v)] over the runs ``offs`` [T+1] of the rows, as one HIP launch and its
    backward as two (csrc/rows_layer_norm.hip).  y and out share a row type (fp32, or bf16 with out and grad_y each rounded once at
    the store); gamma / beta [T,X], the row statistics and both parameter gradients are fp32.  Keeps y, mean and rstd for the
    backward; a call that needs no gradient (torch.no_grad()) passes NULL statistics and saves nothing."""

    @staticmethod
    def forward(ctx, offs, y, gamma, beta, eps, train):
        """``train`` False (the caller runs under torch.no_grad(), or nothing needs a gradient): the statistics are not written."""
        gamma, beta = gamma.contiguous(), beta.contiguous()
        fwd = _k.rows_layer_norm_bf16 if y.dtype == th.bfloat16 else _k.rows_layer_norm
        out, mean, rstd = fwd(offs, y, gamma, beta, eps, save_stats=train)
        if train:
            ctx.save_for_backward(y, gamma, mean, rstd, offs)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        y, gamma, mean, rstd, offs = ctx.saved_tensors
        grad_out = grad_out.contiguous()
        if grad_out.data_ptr() % (4 * grad_out.element_size()):
            grad_out = grad_out.clone()
        bwd = _k.rows_layer_norm_backward_bf16 if y.dtype == th.bfloat16 else _k.rows_layer_norm_backward
        g_y, g_gamma, g_beta = bwd(offs, y, gamma, mean, rstd, grad_out, want_y=ctx.needs_input_grad[1])
        return None, g_y, (g_gamma if ctx.needs_input_grad[2] else None), (g_beta if ctx.needs_input_grad[3] else None), None, None


def typed_layer_norm(y, offs, gamma, beta, eps=1e-5):
    """The per-node-type LayerNorm of HGT's use_norm on the rows y [N, X]: row v of run t of ``offs`` [T+1] is normalised over its
    columns (biased variance, eps inside the root) and meets gamma[t] / beta[t] ([T, X], one pair per run).  On the GPU, for
    contiguous aligned fp32 / bf16 rows of a width that is a multiple of 4 up to 1024, this is TypedLayerNormFunction.  Everything
    else (a width like 10, CPU tensors, non-contiguous or unaligned rows) is a plain torch composition -- F.layer_norm per run,
    in fp32, cast back to y's dtype: correct, not fast."""
    if _typed_layer_norm_kernel_ok(y) and gamma.is_cuda and gamma.dtype == th.float32 and beta.dtype == th.float32:
        train = th.is_grad_enabled() and (y.requires_grad or gamma.requires_grad or beta.requires_grad)
        return TypedLayerNormFunction.apply(offs, y, gamma, beta, float(eps), train)
    bounds = offs.tolist()
    X = y.shape[1]
    parts = [th.nn.functional.layer_norm(y[a:b].float(), (X,), gamma[t].float(), beta[t].float(), eps)
             for t, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])) if b > a]
    return (th.cat(parts, dim=0) if parts else y.float()).to(y.dtype)


def hgt_layer_fused(route, G, h, offs, q_w, a_w, k_lin, v_lin, rel_att, rel_msg, rel_pri, num_heads, fused_attn):
    """The HGT layer [N, out] on path ``fused`` of ``route`` (hgt_route.decide's answer for the call): attention + aggregation as
    one node, then the typed output projection ``a_w`` [T,1,X,out] (one weight per run of offs; the caller folds sigmoid(skip) in)
    -- with ``route.compact_dst`` on the destinations with in-edges only (the other rows of the output are zero by construction).
    A bf16 ``h`` (``route.native_bf16``): h, kv_c, q, new_h, the output and their gradients are bf16 rows, each rounded once where its
    kernel stores it; the parameters, the folded w_kv, lsum, grad_kv_c / grad_q and every parameter gradient stay fp32 (padded head
    columns are dropped with torch ops: dtype-agnostic)."""
    if not _has_single_sided_lists(G):
        G.generate_separate_unique_node_indices_single_sided_for_each_etype()
    st, _ = G.get_rel_node_types()
    w_kv = fold_source_weights(k_lin, v_lin, rel_att, rel_msg, rel_pri, st, num_heads, fused_attn)
    N = h.shape[0]
    d_k, d_pad, groups, Xg = q_w.shape[3] // num_heads, route.d_pad, route.groups, route.Xg
    w_kv, q_w = _pad_heads(w_kv, num_heads, d_k, d_pad, parts=2), _pad_heads(q_w, num_heads, d_k, d_pad)
    dst = _k.destination_lists(G.get_separate_coo_original()["col_indices"], offs)
    dst_lists = dst if route.compact_dst else None
    if groups == 1:
        new_h = HgtAttentionFunction.apply(G, route, num_heads, offs, h, w_kv, q_w, dst_lists)
    else:
        # rows wider than the row kernels take: the heads in `groups` passes (columns of a head group in [k' | m] and in q)
        X, parts = num_heads * d_pad, []
        for i in range(groups):
            w_g = th.cat([w_kv[..., i * Xg:(i + 1) * Xg], w_kv[..., X + i * Xg:X + (i + 1) * Xg]], dim=-1).contiguous()
            parts.append(HgtAttentionFunction.apply(G, route, num_heads // groups, offs, h, w_g, q_w[..., i * Xg:(i + 1) * Xg].contiguous(),
                                                    dst_lists))
        new_h = th.cat(parts, dim=1)
    if d_pad != d_k:
        new_h = new_h.view(new_h.shape[0], num_heads, d_pad)[..., :d_k].reshape(new_h.shape[0], -1)
    if route.out_proj == "bf16_rows":
        return RowsLinearBf16.apply(*((dst[2], dst[0]) if route.compact_dst else (offs, None)), N, new_h, a_w)
    if route.out_proj == "typed_gemm":
        return B_matmul_no_scatter_gather(offs, a_w, new_h)
    if route.out_proj == "rows_scatter":
        return RowsLinearScatter.apply(dst[2], dst[0], N, new_h, a_w)
    out_c = B_matmul_no_scatter_gather(dst[2], a_w, new_h)  # rows of a type are a contiguous piece of the sorted list
    return th.zeros((N, out_c.shape[1]), dtype=out_c.dtype, device=out_c.device).index_copy(0, dst[0], out_c)
