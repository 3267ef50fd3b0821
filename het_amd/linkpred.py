"""Link prediction with a DistMult or a ComplEx head and keyed negatives (opt-in; csrc/triple_score.hip).

The rule.  All key arithmetic is uint64, wrapping; ``sm`` and the stream are those of the keyed sampler and keyed dropout
(DESIGN.md 4.10): ``stream = sm(seed ^ sm(draw))``.

Triples.  A batch has P positives ``(src_i, rel_i, dst_i)`` and K >= 0 negatives per positive: T = P (1 + K) triples
``(s_j, r_j, o_j)``.  ``j < P`` is positive j; ``j = P + m`` with ``m = i K + k`` is the k-th corruption of positive i.  The label is 1
for ``j < P`` and 0 otherwise: it is the position, there is no label tensor.

Keyed corruption (unfiltered)::

    key   = sm(stream + m)
    side  = key >> 63                     0: replace the tail o, 1: replace the head s
    u     = (key >> 31) & 0xFFFFFFFF
    v_old = dst_i if side == 0 else src_i
    [lo, hi) = the run of node_type_offsets that contains v_old   ([0, N) when no offsets are given)
    v_new = lo + ((u * (hi - lo)) >> 32)
    r_j   = rel_i

The replaced end keeps its node type.  N < 2^31, so the product stays below 2^63.  **Unfiltered: v_new == v_old and collisions with
true edges are allowed** -- a different sample than any filtered or torch.randint sampler's for the same seed.  A node of a run of
``hi - lo`` nodes is drawn with a probability that differs from uniform by less than ``(hi - lo) / 2^32``.  An end that lies in no
run (outside [0, N)) is copied as it is.

Score.  ``score_j = sum_d h[s_j, d] * w[r_j, d] * h[o_j, d]`` in fp32; h is [N, D] fp32, or bf16 widened exactly on load; w is [R, D]
fp32; score is [T] fp32.

Gradients for ``g = grad_score`` ([T] fp32), all sums fp32 on widened values:

* ``grad_h[v] = sum_{j: s_j = v} g_j w[r_j] (.) h[o_j] + sum_{j: o_j = v} g_j w[r_j] (.) h[s_j]``; a triple with ``s_j == o_j == v``
  contributes both terms.  Each node's list is summed in ascending slot ``2 j + side`` (side 0: v is the head s_j, side 1: the tail
  o_j); a list longer than L slots (``kernels.triple_long_list()``) is cut into chunks of L from its start, the chunks are summed
  separately and their sums are added in chunk order.  A row without triples is +0.  Every row is written exactly once.  A bf16 h
  gives a bf16 grad_h, rounded once to nearest even after the whole sum.
* ``grad_w[r] = sum_{j: r_j = r} g_j h[s_j] (.) h[o_j]``, in ascending j within chunks of ``triple_params()["rel_chunk"]`` triples
  of the relation's list, then the chunk sums in chunk order.  A relation without triples is +0.  Always fp32.

Ids outside the tables.  A triple with s or o outside [0, N) or r outside [0, R) is **counted, not asserted** (the rule of
SoftmaxCrossEntropy): its score is +0, it contributes to no gradient, the count lands in an int64 on the device
(``DistMultDecoder.last_bad``) and no kernel reads a table through such an id.

Loss.  The head returns scores; the loss over [T] floats stays a torch expression (``link_prediction_loss``: BCE-with-logits
against the implicit labels).  T floats are nothing beside the 2 T D gathered ones, and a score op serves any loss -- a margin, a
softmax over each positive's negatives.

No float atomics anywhere: the same inputs give the same bits on every call, and the autograd node keeps nothing of T D elements.

Filtered ranking (evaluation; csrc/triple_rank.hip; ``distmult_rank``, ``ranking_metrics``).  The rule::

    query j    (a_j, r_j, t_j): anchor node, relation, true node.  Tail ranking of (s, r, o): a = s, t = o.
               Head ranking: a = o, t = s.  DistMult is symmetric, so one kernel serves both.
               sides="both" gives Q = 2 P queries: the P tail queries first, then the P head queries.
    run        [lo_j, hi_j) = the run of node_type_offsets that holds t_j  ([0, N) without offsets)
    q_j[d]     = fl32(h[a_j, d] * w[r_j, d])        h fp32, or bf16 widened on load (exact); w fp32
    score_j(c) = the fp32 fma chain over ascending d, from +0:  acc = fmaf(q_j[d], h[c, d], acc)
    p_j        = score_j(t_j), by the same chain
    excluded   c == t_j; for a tail query every c with (a_j, r_j, c) in the filter set, for a head query every c with
               (c, r_j, a_j) in it; a c listed twice is excluded once; a listed c outside the run changes nothing
    greater_j  = #{ c in run, not excluded : score_j(c) >  p_j }
    equal_j    = #{ c in run, not excluded : score_j(c) == p_j }
    cands_j    = #{ c in run, not excluded }
    bad        a or t outside [0, N), r outside [0, R), or t in no run: **counted, not asserted**.
               greater = equal = cands = 0; no table is read through such an id.
               A filter triple with an id outside its range is ignored.
    rank_j     = 1 + greater_j + equal_j / 2   (fp64, in torch).
               MRR, mean rank and Hits@k (rank_j <= k) are taken over the queries that are not bad.

The chain is the arithmetic of gfx950's fp32 MFMA, which scores the candidates; p_j is a sequential fmaf chain: a candidate whose row
has the bits of the true node's row ties with it exactly.  The three counts are integers added with integer atomics: the same bits on
every call.  The ``[Q, N]`` score matrix never exists.  **The filter serves evaluation only: training negatives stay unfiltered.**
The pairs (query, excluded candidate) of a batch come from two ``searchsorted`` and one expansion in torch over a ``FilterIndex``
built once; the expansion needs the pair count on the host -- **the one read-back of a ranking call** (none without a filter).

The ComplEx head (``ComplExDecoder``, ``complex_rank``).  DistMult's score is symmetric in s and o: it gives a triple
and its reverse the same score to the bit.  ComplEx is the smallest trilinear decoder without that defect.  Layout: ``h [N, D]`` and
``w [R, D]`` with D even; column 2k is the real part of component k and column 2k + 1 the imaginary part
(``torch.view_as_complex(x.view(-1, D // 2, 2))``).  With ``a = h[s_j]``, ``b = w[r_j]``, ``c = h[o_j]``, per component (a_r, a_i) and
so on, and ``g = grad_score_j``::

    score_j    = sum_k Re(a_k * b_k * conj(c_k))
               = sum_k (a_r b_r - a_i b_i) c_r + (a_r b_i + a_i b_r) c_i
    grad a_r  += g (b_r c_r + b_i c_i)      grad a_i += g (b_r c_i - b_i c_r)      (slot side 0: v is the head s_j)
    grad c_r  += g (a_r b_r - a_i b_i)      grad c_i += g (a_r b_i + a_i b_r)      (slot side 1: v is the tail o_j)
    grad b_r  += g (a_r c_r + a_i c_i)      grad b_i += g (a_r c_i - a_i c_r)

Everything else is the DistMult head's, to the letter: slots ascending ``2 j + side``, lists longer than L summed in chunks of L with the
chunk sums added in chunk order, grad_w in chunks of the relation chunk, every grad_h and grad_w row written exactly once (+0 where a
list is empty), a bf16 grad_h rounded once after the whole sum, a bad id **counted, not asserted** and never an address, a triple with
``s == o`` in both slots, no float atomics, no zero-fill, no read-back, the same bits on every call.  The plan and the workspaces are the
DistMult head's own.  The native widths are the multiples of 4 of ``kernels.triple_params()``: a 16-byte piece of a row is two whole
complex numbers.

ComplEx ranking.  A query is ``(a_j, r_j, t_j, side_j)``: side 0 ranks tails (the anchor is the head s, the candidates stand in o's
place), side 1 ranks heads (the anchor is the tail o, the candidates stand in s's place); any other side makes the query bad.  Unlike
DistMult the two sides need different q; with ``x = h[a_j]``, ``b = w[r_j]``::

    side 0:   q_j[2k] = fl32(fl32(x_r b_r) - fl32(x_i b_i))     q_j[2k+1] = fl32(fl32(x_r b_i) + fl32(x_i b_r))
    side 1:   q_j[2k] = fl32(fl32(b_r x_r) + fl32(b_i x_i))     q_j[2k+1] = fl32(fl32(b_r x_i) - fl32(b_i x_r))
    score_j(c) = the fp32 fma chain over ascending d, from +0:  acc = fmaf(q_j[d], h[c, d], acc);   p_j = score_j(t_j), the same chain

Each q element is three separately rounded fp32 operations, never a fused multiply-add: float32 arithmetic in numpy or torch gives the
same bits.  The run, the exclusions, the three counts, the bad queries and the metrics follow the DistMult rule above unchanged; the
rank pass is the same launch (it reads q, never w).
"""
from __future__ import annotations

import collections

import torch as th
import torch.nn as nn

from . import kernels as _k
from ._lib import HetError
from .layers import _M64, _i64, _lsr, _sm_tensor


def _stream(seed: int, draw: int) -> int:
    from .sampling import _sm_int
    return _sm_int((int(seed) & _M64) ^ _sm_int(int(draw) & _M64))


def _keyed_corruptions_torch(src, rel, dst, K, seed, draw, offs, N):
    """The rule in torch int64 arithmetic on any device: the bits het_triple_corrupt gives."""
    P = src.shape[0]
    m = th.arange(P * K, dtype=th.int64, device=src.device)
    key = _sm_tensor(m + _i64(_stream(seed, draw)))
    head = _lsr(key, 63) == 1
    u = _lsr(key, 31) & 0xFFFFFFFF
    i = th.div(m, max(K, 1), rounding_mode="floor")
    si, ri, oi = src[i], rel[i], dst[i]
    v_old = th.where(head, si, oi)
    if offs is None:
        inside = (v_old >= 0) & (v_old < N)
        lo, span = th.zeros_like(v_old), th.full_like(v_old, N)
    else:
        inside = (v_old >= offs[0]) & (v_old < offs[-1])
        ty = (th.searchsorted(offs[:-1].contiguous(), v_old, right=True) - 1).clamp_(0, offs.numel() - 2)
        lo = offs[ty]
        span = offs[ty + 1] - lo
    v_new = th.where(inside, lo + ((u * span) >> 32), v_old)
    return (th.cat([src, th.where(head, v_new, si)]), th.cat([rel, ri]), th.cat([dst, th.where(head, oi, v_new)]))


def keyed_corruptions(src, rel, dst, num_neg: int, *, seed: int, draw: int, node_type_offsets=None, num_nodes: int):
    """(s, r, o), each [P (1 + num_neg)] int64: the P positives followed by ``num_neg`` keyed corruptions of each (the module's rule;
    **unfiltered: a corruption may equal its positive or another true edge**).  One HIP launch on CUDA tensors; on the CPU, or
    where the library is absent, a torch implementation gives the same bits."""
    num_neg, num_nodes = int(num_neg), int(num_nodes)
    if num_neg < 0:
        raise ValueError(f"keyed_corruptions: num_neg={num_neg} (at least 0)")
    if not 0 <= num_nodes < 2 ** 31:
        raise ValueError(f"keyed_corruptions: num_nodes={num_nodes} (0 <= num_nodes < 2^31)")
    if not (src.dim() == rel.dim() == dst.dim() == 1 and src.shape == rel.shape == dst.shape):
        raise ValueError(f"keyed_corruptions: src, rel and dst are 1-d tensors of one length, got {tuple(src.shape)}, {tuple(rel.shape)}, "
                         f"{tuple(dst.shape)}")
    src, rel, dst = (t.detach().to(th.int64).contiguous() for t in (src, rel, dst))
    offs = None
    if node_type_offsets is not None:
        offs = th.as_tensor(node_type_offsets).detach().to(device=src.device, dtype=th.int64).contiguous()
        if offs.dim() != 1 or offs.numel() < 2:
            raise ValueError(f"keyed_corruptions: node_type_offsets [num_types + 1], got {tuple(offs.shape)}")
    if src.shape[0] * (1 + num_neg) >= 2 ** 30:
        raise ValueError(f"keyed_corruptions: {src.shape[0]} positives with {num_neg} negatives each are 2^30 triples or more")
    if src.is_cuda and _native_available():
        return _k.triple_corrupt(src, rel, dst, num_neg, seed, draw, offs, num_nodes)
    return _keyed_corruptions_torch(src, rel, dst, num_neg, seed, draw, offs, num_nodes)


def _native_available() -> bool:
    try:
        from . import _lib
        _lib.lib()
        return True
    except HetError:
        return False


def keyed_positive_edges(g, batch_size: int, *, seed: int, draw: int):
    """(src, rel, dst), each [batch_size] int64: edges of ``g`` drawn with replacement from its separate COO (relation-major), position
    ``e_i = (((sm(stream + i) >> 31) & 0xFFFFFFFF) * E) >> 32`` with the stream of (seed, draw); E < 2^31.  Torch only: P elements."""
    coo = g.get_separate_coo_original()
    rel_ptrs, row, col = coo["rel_ptrs"], coo["row_indices"], coo["col_indices"]
    E = int(row.shape[0])
    if not 0 < E < 2 ** 31:
        raise ValueError(f"keyed_positive_edges: a graph of {E} edges (0 < E < 2^31)")
    i = th.arange(int(batch_size), dtype=th.int64, device=row.device)
    key = _sm_tensor(i + _i64(_stream(seed, draw)))
    e = ((_lsr(key, 31) & 0xFFFFFFFF) * E) >> 32
    rel = th.searchsorted(rel_ptrs.to(row.device).contiguous(), e, right=True) - 1
    return row[e], rel, col[e]


def _count_bad(s, r, o, N, R):
    return (((s < 0) | (s >= N) | (o < 0) | (o >= N) | (r < 0) | (r >= R)).sum()).reshape(1)


def distmult_score_torch(h, w, s, r, o):
    """(score [T] fp32 (fp64 for fp64 tables), bad [1] int64) of the module's rule as a differentiable torch composition: correct, not
    fast -- three [T, D] gathers, two [T, D] products kept for the backward, an index_add_ in it."""
    N, R = h.shape[0], w.shape[0]
    ok = (s >= 0) & (s < N) & (o >= 0) & (o < N) & (r >= 0) & (r < R)
    zero = th.zeros_like(s)
    acc = th.float64 if h.dtype == th.float64 else th.float32
    hf = h.to(acc)  # (widened before the gathers: the backward's index_add_ then sums in fp32 and a bf16 grad_h is rounded once)
    hs, ho, wr = hf[th.where(ok, s, zero)], hf[th.where(ok, o, zero)], w[th.where(ok, r, zero)].to(acc)
    score = (hs * wr * ho).sum(-1)
    return th.where(ok, score, th.zeros((), dtype=acc, device=h.device)), (~ok).sum().reshape(1)


def _complex_parts(x):
    return x[..., 0::2], x[..., 1::2]


def complex_score_torch(h, w, s, r, o):
    """(score [T] fp32 (fp64 for fp64 tables), bad [1] int64) of the module's ComplEx rule as a differentiable torch composition:
    correct, not fast -- three [T, D] gathers and a dozen [T, D / 2] products kept for the backward.  The CPU and odd-dtype fallback."""
    N, R = h.shape[0], w.shape[0]
    if h.dim() != 2 or w.dim() != 2 or h.shape[1] != w.shape[1] or h.shape[1] % 2:
        raise ValueError(f"complex_score_torch: h [N, D] and w [R, D] with D even, got {tuple(h.shape)} and {tuple(w.shape)}")
    ok = (s >= 0) & (s < N) & (o >= 0) & (o < N) & (r >= 0) & (r < R)
    zero = th.zeros_like(s)
    acc = th.float64 if h.dtype == th.float64 else th.float32
    hf = h.to(acc)  # (widened before the gathers: the backward's index_add_ then sums in fp32 and a bf16 grad_h is rounded once)
    (ar, ai), (cr, ci) = _complex_parts(hf[th.where(ok, s, zero)]), _complex_parts(hf[th.where(ok, o, zero)])
    br, bi = _complex_parts(w[th.where(ok, r, zero)].to(acc))
    score = ((ar * br - ai * bi) * cr + (ar * bi + ai * br) * ci).sum(-1)
    return th.where(ok, score, th.zeros((), dtype=acc, device=h.device)), (~ok).sum().reshape(1)


def _aligned_rows(t):
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=th.contiguous_format)


class DistMultScoreFunction(th.autograd.Function):
    """(score, bad) = the DistMult scores of the triples (s, r, o) over the rows ``h`` and the relation vectors ``w`` as one autograd
    node on the HIP kernels: one launch forward; the plan of the batch (sorts and searches on the device, no read-back) is built in the
    forward only when a gradient is needed; the backward is node-major and relation-major, without float atomics.  Saved for the
    backward: h, w, the ids and the plan -- nothing of T D elements.  ``bad`` (int64 [1]) is not differentiable.  Tensors the kernels
    do not take raise HetError (DistMultDecoder routes those to the torch composition).  A double backward is refused:
    the backward is once_differentiable."""

    @staticmethod
    def forward(ctx, h, w, s, r, o):
        return _score_forward(ctx, "DistMultScoreFunction", _k._distmult_chk, _k._distmult_score, h, w, s, r, o)

    @staticmethod
    @th.autograd.function.once_differentiable
    def backward(ctx, grad_score, _grad_bad):
        return _score_backward(ctx, _k._distmult_score_backward, grad_score)


class ComplExScoreFunction(th.autograd.Function):
    """(score, bad) = the ComplEx scores of the triples (s, r, o) (the module's rule) as one autograd node on the HIP kernels, with
    DistMultScoreFunction's contract: one launch forward, the plan built only when a gradient is needed, a node-major and
    relation-major backward without float atomics; saved: h, w, the ids and the plan -- nothing of T D elements.  ``bad`` is not
    differentiable; tensors the kernels do not take raise HetError; a double backward is refused (once_differentiable)."""

    @staticmethod
    def forward(ctx, h, w, s, r, o):
        return _score_forward(ctx, "ComplExScoreFunction", _k._complex_chk, _k._complex_score, h, w, s, r, o)

    @staticmethod
    @th.autograd.function.once_differentiable
    def backward(ctx, grad_score, _grad_bad):
        return _score_backward(ctx, _k._complex_score_backward, grad_score)


def _score_forward(ctx, name, chk, score_fn, h, w, s, r, o):
    """The forward of both score nodes: ``chk`` and ``score_fn`` are the decoder's check and score launch of het_amd.kernels."""
    hd, wd = _aligned_rows(h.detach()), _aligned_rows(w.detach())  # (a strided or misaligned table: the kernels run on a copy)
    ids = tuple(t.detach().to(th.int64).contiguous() for t in (s, r, o))
    chk(name, hd, wd, *ids)
    want_h, want_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    score = score_fn(hd, wd, *ids)
    if want_h or want_w:
        plan = _k._triple_plan(*ids, hd.shape[0], wd.shape[0])
        bad = plan.bad
        ctx.ids, ctx.plan = ids, plan  # (index tensors: nothing autograd tracks, and nothing an inference-mode id would break)
        ctx.save_for_backward(hd, wd)
    else:
        bad = _count_bad(*ids, hd.shape[0], wd.shape[0])
    ctx.mark_non_differentiable(bad)
    ctx.set_materialize_grads(False)
    return score, bad


def _score_backward(ctx, backward_fn, grad_score):
    want_h, want_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    if grad_score is None or not (want_h or want_w):
        return None, None, None, None, None
    hd, wd = ctx.saved_tensors
    g = grad_score.detach().to(device=hd.device, dtype=th.float32).contiguous()
    grad_h, grad_w = backward_fn(hd, wd, *ctx.ids, g, ctx.plan, want_h, want_w)
    return grad_h, grad_w, None, None, None


class DistMultDecoder(nn.Module):
    """The DistMult head: ``forward(h, s, r, o)`` returns the [T] fp32 scores of the triples over the node rows ``h`` [N, dim] and the
    module's ``w_relation`` [num_rels, dim] (fp32, xavier-uniform).  Labels are implicit in the position (the module docstring);
    ``link_prediction_loss`` is the usual loss, any other expression of the scores works as well.

    A triple with an id outside its table is **counted, not asserted**: its score is +0 and it gets no gradient.  ``last_bad`` holds
    the count of the last call as an int64 [1] device tensor; ``check_ids=True`` reads it back after every call -- the module's only
    host synchronisation -- and raises ValueError on a non-zero count.

    Contiguous or strided float32 / bfloat16 GPU rows of a native width (``kernels.distmult_ok``) take the HIP kernels
    (DistMultScoreFunction); everything else -- CPU tensors, fp16 / fp64, a ``dim`` that is no multiple of 4 -- and every call of a
    module built with ``native=False`` (an ``h`` that needs a double backward) takes the torch composition of the same rule: correct, not
    faster."""

    _function = DistMultScoreFunction  # (what ComplExDecoder replaces: the native node, the torch composition, the ranking call)
    _score_torch = staticmethod(distmult_score_torch)

    def __init__(self, num_rels: int, dim: int, check_ids: bool = False, native: bool = True):
        super().__init__()
        self.num_rels, self.dim, self.check_ids, self.native = int(num_rels), int(dim), bool(check_ids), bool(native)
        self.w_relation = nn.Parameter(th.empty(self.num_rels, self.dim, dtype=th.float32))
        nn.init.xavier_uniform_(self.w_relation)
        self.last_bad = None

    def extra_repr(self):
        return f"num_rels={self.num_rels}, dim={self.dim}, check_ids={self.check_ids}, native={self.native}"

    def takes_native(self, h) -> bool:
        """Whether a call with these rows runs the HIP kernels."""
        w = self.w_relation
        return (self.native and h.is_cuda and w.device == h.device and h.dim() == 2 and h.dtype in (th.float32, th.bfloat16)
                and w.dtype == th.float32 and _k.triple_width_ok(h.shape[1]) and h.shape[0] < 2 ** 31 - 1 and _native_available())

    def forward(self, h, s, r, o):
        name = type(self).__name__
        if h.dim() != 2 or h.shape[1] != self.dim:
            raise ValueError(f"{name}: h [N, {self.dim}], got {tuple(h.shape)}")
        if not (s.dim() == r.dim() == o.dim() == 1 and s.shape == r.shape == o.shape):
            raise ValueError(f"{name}: s, r and o are 1-d id tensors of one length, got {tuple(s.shape)}, {tuple(r.shape)}, {tuple(o.shape)}")
        if any(t.is_floating_point() or t.dtype == th.bool for t in (s, r, o)):
            raise ValueError(f"{name}: integer ids expected")
        if s.shape[0] >= 2 ** 30:
            raise ValueError(f"{name}: {s.shape[0]} triples (fewer than 2^30)")
        if self.takes_native(h):
            score, bad = self._function.apply(h, self.w_relation, s, r, o)
        else:
            score, bad = self._score_torch(h, self.w_relation, *(t.to(th.int64) for t in (s, r, o)))
            score = score.to(th.float32)
        self.last_bad = bad.detach()
        if self.check_ids:
            n_bad = int(bad)
            if n_bad:
                raise ValueError(f"{name}: {n_bad} triple(s) have an id outside [0, {h.shape[0]}) nodes or [0, {self.num_rels}) relations")
        return score

    def rank(self, h, s, r, o, **kw):
        """``distmult_rank(h, self.w_relation, s, r, o, **kw)``: the filtered ranks of the triples under this head (no gradient; a module
        built with ``native=False`` takes the torch composition)."""
        if h.dim() != 2 or h.shape[1] != self.dim:
            raise ValueError(f"{type(self).__name__}: h [N, {self.dim}], got {tuple(h.shape)}")
        kw.setdefault("native", self.native)
        return self._rank(h, self.w_relation, s, r, o, **kw)

    @staticmethod
    def _rank(h, w, s, r, o, **kw):
        return distmult_rank(h, w, s, r, o, **kw)


class ComplExDecoder(DistMultDecoder):
    """The ComplEx head: DistMultDecoder's surface (``forward(h, s, r, o)``, ``last_bad``, ``check_ids``, ``takes_native``, ``rank``,
    ``w_relation`` [num_rels, dim] fp32 xavier-uniform) with the module's ComplEx rule: ``dim`` is even, column 2k the real and
    2k + 1 the imaginary part of component k, and ``score(s, r, o) != score(o, r, s)`` in general.  Rows of a native width (a
    multiple of 4, ``kernels.complex_ok``) take the HIP kernels (ComplExScoreFunction); everything else, and ``native=False``, takes
    ``complex_score_torch``."""
    _function = ComplExScoreFunction
    _score_torch = staticmethod(complex_score_torch)

    def __init__(self, num_rels: int, dim: int, check_ids: bool = False, native: bool = True):
        if int(dim) % 2:
            raise ValueError(f"ComplExDecoder: dim={dim} (even: pairs of a real and an imaginary column)")
        super().__init__(num_rels, dim, check_ids=check_ids, native=native)

    @staticmethod
    def _rank(h, w, s, r, o, **kw):
        return complex_rank(h, w, s, r, o, **kw)


def link_prediction_loss(scores, num_pos: int):
    """Mean binary cross-entropy with logits of ``scores`` [T] against the implicit labels: 1 for the first ``num_pos``, 0 after."""
    num_pos = int(num_pos)
    if scores.dim() != 1 or not 0 <= num_pos <= scores.shape[0]:
        raise ValueError(f"link_prediction_loss: scores [T] and 0 <= num_pos <= T, got {tuple(scores.shape)} and {num_pos}")
    labels = th.zeros_like(scores)
    labels[:num_pos] = 1.0
    return nn.functional.binary_cross_entropy_with_logits(scores, labels)


# ---- filtered ranking (evaluation): the rule in the module docstring -------------------------------------------------------------
RankResult = collections.namedtuple("RankResult", "greater equal candidates bad")
RankResult.__doc__ = """What ``distmult_rank`` returns, one entry per query: ``greater``, ``equal`` and ``candidates`` int32 [Q] (the rule's three
counts) and ``bad`` bool [Q] (the queries with an id outside its table or a true node in no run: their counts are 0 and
``ranking_metrics`` leaves them out; ``bad.sum()`` is the count the kernel keeps on the device)."""


class FilterIndex:
    """The known triples of a graph as two sorted key arrays, built once in torch: ``tail_keys`` = ``r * N + s`` with ``tail_vals`` = o
    (the known tails of (s, r)), ``head_keys`` = ``r * N + o`` with ``head_vals`` = s (the known heads of (r, o)); both stable-sorted by
    key.  A triple with an id outside [0, num_nodes) or [0, num_rels) is ignored; duplicates are kept (they exclude once)."""

    def __init__(self, s, r, o, num_nodes: int, num_rels: int):
        N, R = int(num_nodes), int(num_rels)
        if not (0 <= N < 2 ** 31 - 1 and 0 <= R < 2 ** 31 - 1):
            raise ValueError(f"FilterIndex: num_nodes={N}, num_rels={R} (both below 2^31 - 1)")
        if not (s.dim() == r.dim() == o.dim() == 1 and s.shape == r.shape == o.shape):
            raise ValueError(f"FilterIndex: s, r and o are 1-d id tensors of one length, got {tuple(s.shape)}, {tuple(r.shape)}, {tuple(o.shape)}")
        with th.no_grad():
            s, r, o = (t.detach().to(th.int64) for t in (s, r, o))
            ok = (s >= 0) & (s < N) & (o >= 0) & (o < N) & (r >= 0) & (r < R)
            s, r, o = s[ok], r[ok], o[ok]
            tk, ti = th.sort(r * N + s, stable=True)
            hk, hi = th.sort(r * N + o, stable=True)
            self._set(tk, o[ti], hk, s[hi], N, R)

    def _set(self, tk, tv, hk, hv, N, R):
        self.num_nodes, self.num_rels = N, R
        self._keys = th.cat([tk, hk + R * N]).contiguous()  # one array for one searchsorted: the head keys lie behind every tail key
        self._vals = th.cat([tv, hv]).contiguous()
        E = tk.shape[0]
        self.tail_keys, self.tail_vals, self.head_keys, self.head_vals = self._keys[:E], self._vals[:E], hk, self._vals[E:]

    @classmethod
    def from_graph(cls, g):
        """The index of the graph's own edges (its separate COO, relation-major: row = s, col = o)."""
        coo = g.get_separate_coo_original()
        rel_ptrs, row, col = coo["rel_ptrs"].to(coo["row_indices"].device), coo["row_indices"], coo["col_indices"]
        R = int(rel_ptrs.numel()) - 1
        rel = th.repeat_interleave(th.arange(R, dtype=th.int64, device=row.device), rel_ptrs[1:] - rel_ptrs[:-1], output_size=int(row.shape[0]))
        return cls(row, rel, col, g.get_num_nodes(), R)

    @property
    def device(self):
        return self._keys.device

    def to(self, device):
        device = th.device(device)
        if self._keys.device == device:
            return self
        new = object.__new__(FilterIndex)
        new._set(self.tail_keys.to(device), self.tail_vals.to(device), self.head_keys.to(device), self.head_vals.to(device), self.num_nodes,
                 self.num_rels)
        return new

    def pairs(self, anchor, rel, head):
        """(pair_query, pair_cand), int64 [n] each: for query j every known c -- the tails of (anchor_j, rel_j) where ``head[j]`` is
        False, the heads of (rel_j, anchor_j) where it is True -- in query order.  Two searchsorted and one expansion; the expansion's
        length is **read back to the host**: the one synchronisation of a filtered ranking call."""
        N, R = self.num_nodes, self.num_rels
        Q, dev = anchor.shape[0], anchor.device
        ok = (anchor >= 0) & (anchor < N) & (rel >= 0) & (rel < R)
        key = th.where(ok, rel * N + anchor + head.to(th.int64) * (R * N), th.full_like(anchor, -1))
        lo = th.searchsorted(self._keys, key)
        cnt = th.searchsorted(self._keys, key, right=True) - lo
        total = int(cnt.sum())  # (the read-back)
        if total == 0:
            e = th.zeros(0, dtype=th.int64, device=dev)
            return e, e.clone()
        qi = th.repeat_interleave(th.arange(Q, dtype=th.int64, device=dev), cnt, output_size=total)
        first = th.cumsum(cnt, 0) - cnt
        pos = th.arange(total, dtype=th.int64, device=dev) - first[qi] + lo[qi]
        return qi, self._vals[pos]


def _rank_queries(s, r, o, sides, name="distmult_rank"):
    """(anchor, rel, truth, head) of the rule: the tail queries, the head queries, or the tail queries followed by the head queries."""
    f = th.zeros(s.shape[0], dtype=th.bool, device=s.device)
    if sides == "tail":
        return s, r, o, f
    if sides == "head":
        return o, r, s, ~f
    if sides == "both":
        return th.cat([s, o]), th.cat([r, r]), th.cat([o, s]), th.cat([f, ~f])
    raise ValueError(f"{name}: sides is 'both', 'tail' or 'head', got {sides!r}")


def _rank_prepare(name, h, w, s, r, o, sides, filter, node_type_offsets, with_head=False):
    """Checks, then (anchor, rel, truth, lo, hi, bad, offsets, pair_query, pair_cand) on h's device; ``with_head``: and the side of every
    query (bool: True ranks heads)."""
    if h.dim() != 2 or w.dim() != 2 or h.shape[1] != w.shape[1] or not (h.is_floating_point() and w.is_floating_point()):
        raise ValueError(f"{name}: floating-point h [N, D] and w [R, D], got {h.dtype} {tuple(h.shape)} and {w.dtype} {tuple(w.shape)}")
    if not (s.dim() == r.dim() == o.dim() == 1 and s.shape == r.shape == o.shape):
        raise ValueError(f"{name}: s, r and o are 1-d id tensors of one length, got {tuple(s.shape)}, {tuple(r.shape)}, {tuple(o.shape)}")
    if any(t.is_floating_point() or t.dtype == th.bool for t in (s, r, o)):
        raise ValueError(f"{name}: integer ids expected")
    N, R, dev = h.shape[0], w.shape[0], h.device
    if w.device != dev:
        raise ValueError(f"{name}: h on {dev} and w on {w.device}")
    if not (N < 2 ** 31 - 1 and R < 2 ** 31 - 1 and 2 * s.shape[0] < 2 ** 30):
        raise ValueError(f"{name}: {N} nodes, {R} relations (both below 2^31 - 1), {s.shape[0]} triples (fewer than 2^29)")
    a, rr, t, head = _rank_queries(*(x.detach().to(device=dev, dtype=th.int64) for x in (s, r, o)), sides, name)
    a, rr, t = a.contiguous(), rr.contiguous(), t.contiguous()
    offs = None
    if node_type_offsets is not None:
        offs = th.as_tensor(node_type_offsets).detach().to(device=dev, dtype=th.int64).contiguous()
        if offs.dim() != 1 or offs.numel() < 2:
            raise ValueError(f"{name}: node_type_offsets [num_types + 1], got {tuple(offs.shape)}")
    inrun = (t >= 0) & (t < N)
    lo, hi = th.zeros_like(t), th.full_like(t, N)
    if offs is not None:
        inrun &= (t >= offs[0]) & (t < offs[-1])
        ty = (th.searchsorted(offs[:-1].contiguous(), t, right=True) - 1).clamp_(0, offs.numel() - 2)
        lo, hi = offs[ty].clamp(min=0), offs[ty + 1].clamp(max=N)
    bad = ~(inrun & (a >= 0) & (a < N) & (rr >= 0) & (rr < R))
    pq = pc = None
    if filter is not None:
        if not isinstance(filter, FilterIndex) or (filter.num_nodes, filter.num_rels) != (N, R):
            raise ValueError(f"{name}: filter is a FilterIndex over {N} nodes and {R} relations")
        pq, pc = filter.to(dev).pairs(a, rr, head)
    if with_head:
        return a, rr, t, lo, hi, bad, offs, pq, pc, head
    return a, rr, t, lo, hi, bad, offs, pq, pc


def _complex_q(x, b, head):
    """q of the ComplEx ranking rule: every product and every sum is its own torch operation, so each is rounded on its own."""
    (xr, xi), (br, bi) = _complex_parts(x), _complex_parts(b)
    q = th.empty_like(x)
    q[:, 0::2] = th.where(head[:, None], br * xr + bi * xi, xr * br - xi * bi)
    q[:, 1::2] = th.where(head[:, None], br * xi - bi * xr, xr * bi + xi * br)
    return q


def _rank_torch(h, w, a, rr, t, lo, hi, bad, pq, pc, chunk, head=None):
    """``head`` (bool [Q]): the ComplEx rule's q for these sides; None: DistMult's."""
    acc = th.float64 if h.dtype == th.float64 else th.float32
    N, Q, dev = h.shape[0], a.shape[0], h.device
    zero = th.zeros_like(a)
    lo, hi = th.where(bad, zero, lo), th.where(bad, zero, hi)
    if head is None:
        q = h[th.where(bad, zero, a)].to(acc) * w[th.where(bad, zero, rr)].to(acc)  # (the rounded product)
    else:
        q = _complex_q(h[th.where(bad, zero, a)].to(acc), w[th.where(bad, zero, rr)].to(acc), head)
    p = (q * h[th.where(bad, zero, t)].to(acc)).sum(-1) if N else th.zeros(Q, dtype=acc, device=dev)
    out = th.zeros(3, Q, dtype=th.int64, device=dev)
    for c0 in range(0, N, chunk):
        c1 = min(N, c0 + chunk)
        sc = q @ h[c0:c1].to(acc).t()
        c = th.arange(c0, c1, dtype=th.int64, device=dev)[None]
        valid = (c >= lo[:, None]) & (c < hi[:, None]) & (c != t[:, None])
        if pq is not None and pq.numel():
            sel = (pc >= c0) & (pc < c1)
            valid[pq[sel], pc[sel] - c0] = False
        out[0] += (valid & (sc > p[:, None])).sum(1)
        out[1] += (valid & (sc == p[:, None])).sum(1)
        out[2] += valid.sum(1)
    out = out.to(th.int32)
    return RankResult(out[0], out[1], out[2], bad)


def distmult_rank_torch(h, w, s, r, o, *, sides: str = "both", filter=None, node_type_offsets=None, chunk: int = 65536):
    """``distmult_rank`` as a torch composition of the same rule, chunked over ``chunk`` candidates: q as the rounded product, one
    [Q, chunk] matmul per chunk, the same masks (the filter as an index_put_ into the chunk's mask).  Correct, not fast; the order of
    the sums is the matmul's, so on inputs that are not exactly representable a near-tie may fall on the other side than in the
    kernels.  It serves CPU tensors, fp16 / fp64 tables, widths the kernels do not take and ``native=False``."""
    with th.no_grad():
        h, w = h.detach(), w.detach()
        a, rr, t, lo, hi, bad, _, pq, pc = _rank_prepare("distmult_rank_torch", h, w, s, r, o, sides, filter, node_type_offsets)
        return _rank_torch(h, w, a, rr, t, lo, hi, bad, pq, pc, max(1, int(chunk)))


def distmult_rank(h, w, s, r, o, *, sides: str = "both", filter=None, node_type_offsets=None, native: bool = True):
    """The filtered ranks of the triples (s, r, o) under the DistMult score of the rows ``h`` [N, D] and the relation vectors ``w`` [R, D]
    (the module's rule): ``RankResult(greater, equal, candidates, bad)``, one entry per query -- ``sides="both"``: the P tail queries
    (rank o among the tails of (s, r)), then the P head queries; ``"tail"`` / ``"head"``: one of them.  ``filter``: a ``FilterIndex`` of
    the known triples (None: only the true node is excluded -- the raw setting); ``node_type_offsets``: candidates are the nodes of the
    true node's type.

    Runs under ``no_grad`` and keeps nothing: inputs that require grad are detached, the counts carry no graph.  Contiguous or strided
    float32 / bfloat16 GPU rows of a width of ``kernels.triple_rank_params()`` take the HIP kernels (a strided or misaligned table
    runs on a copy): a prelude, with a filter a sort of the pairs, one MFMA pass that reads ``h`` once and stores no score.  Everything
    else, and ``native=False``, takes ``distmult_rank_torch``.  With a filter the pair count is read back once (``FilterIndex.pairs``)."""
    with th.no_grad():
        h, w = h.detach(), w.detach()
        a, rr, t, lo, hi, bad, offs, pq, pc = _rank_prepare("distmult_rank", h, w, s, r, o, sides, filter, node_type_offsets)
        if (native and h.is_cuda and h.dtype in (th.float32, th.bfloat16) and w.dtype == th.float32 and _native_available()):
            hd, wd = _aligned_rows(h), _aligned_rows(w)
            if _k.triple_rank_ok(hd, wd):
                if pq is not None and pq.numel() == 0:
                    pq = pc = None
                inv = None
                if offs is not None and a.shape[0] > 1:  # queries of one type side by side: a query tile then skips the other types' tiles
                    order = th.sort(lo, stable=True).indices
                    inv = th.empty_like(order)
                    inv[order] = th.arange(order.shape[0], dtype=th.int64, device=order.device)
                    a, rr, t = a[order], rr[order], t[order]
                    pq = None if pq is None else inv[pq]
                g, e, c, _ = _k.triple_rank(hd, wd, a, rr, t, pq, pc, offs)
                if inv is not None:
                    g, e, c = g[inv], e[inv], c[inv]
                return RankResult(g, e, c, bad)
        return _rank_torch(h, w, a, rr, t, lo, hi, bad, pq, pc, 65536)


def complex_rank_torch(h, w, s, r, o, *, sides: str = "both", filter=None, node_type_offsets=None, chunk: int = 65536):
    """``complex_rank`` as a torch composition of the same rule, chunked over ``chunk`` candidates: ``distmult_rank_torch`` with the
    ComplEx rule's q (three separately rounded operations per element).  Correct, not fast; the order of the sums is the matmul's."""
    with th.no_grad():
        h, w = h.detach(), w.detach()
        if h.dim() == 2 and h.shape[1] % 2:
            raise ValueError(f"complex_rank_torch: h [N, D] with D even, got {tuple(h.shape)}")
        a, rr, t, lo, hi, bad, _, pq, pc, head = _rank_prepare("complex_rank_torch", h, w, s, r, o, sides, filter, node_type_offsets, True)
        return _rank_torch(h, w, a, rr, t, lo, hi, bad, pq, pc, max(1, int(chunk)), head)


def complex_rank(h, w, s, r, o, *, sides: str = "both", filter=None, node_type_offsets=None, native: bool = True):
    """The filtered ranks of the triples (s, r, o) under the ComplEx score (the module's rule): ``distmult_rank``'s arguments, routes and
    ``RankResult``.  A tail query ranks c by score(s, r, c), a head query by score(c, r, o): the two differ, so the prelude forms q by
    the side of the query; the sort of the pairs and the MFMA pass are the DistMult head's launches.  ``FilterIndex.pairs`` is already
    directional.  Everything the kernels do not take, and ``native=False``, takes ``complex_rank_torch``."""
    with th.no_grad():
        h, w = h.detach(), w.detach()
        if h.dim() == 2 and h.shape[1] % 2:
            raise ValueError(f"complex_rank: h [N, D] with D even, got {tuple(h.shape)}")
        a, rr, t, lo, hi, bad, offs, pq, pc, head = _rank_prepare("complex_rank", h, w, s, r, o, sides, filter, node_type_offsets, True)
        if (native and h.is_cuda and h.dtype in (th.float32, th.bfloat16) and w.dtype == th.float32 and _native_available()):
            hd, wd = _aligned_rows(h), _aligned_rows(w)
            if _k.triple_rank_ok(hd, wd):
                if pq is not None and pq.numel() == 0:
                    pq = pc = None
                side = head.to(th.int64)
                inv = None
                if offs is not None and a.shape[0] > 1:  # queries of one type side by side: a query tile then skips the other types' tiles
                    order = th.sort(lo, stable=True).indices
                    inv = th.empty_like(order)
                    inv[order] = th.arange(order.shape[0], dtype=th.int64, device=order.device)
                    a, rr, t, side = a[order], rr[order], t[order], side[order]
                    pq = None if pq is None else inv[pq]
                g, e, c, _ = _k.complex_rank(hd, wd, a, rr, t, side, pq, pc, offs)
                if inv is not None:
                    g, e, c = g[inv], e[inv], c[inv]
                return RankResult(g, e, c, bad)
        return _rank_torch(h, w, a, rr, t, lo, hi, bad, pq, pc, 65536, head)


def ranking_metrics(result, ks=(1, 3, 10)):
    """{"mrr", "mean_rank", "hits@k" for k in ks, "queries"} of a ``RankResult``: ``rank = 1 + greater + equal / 2`` in fp64 (a tie
    counts half), the means over the queries that are not bad; NaN means with no such query.  Reads the result back."""
    with th.no_grad():
        good = ~result.bad
        rank = (1.0 + result.greater.to(th.float64) + result.equal.to(th.float64) / 2)[good]
        n = int(rank.numel())
        nan = float("nan")
        out = {"mrr": float((1.0 / rank).mean()) if n else nan, "mean_rank": float(rank.mean()) if n else nan}
        for k in ks:
            out[f"hits@{int(k)}"] = float((rank <= int(k)).to(th.float64).mean()) if n else nan
        out["queries"] = n
        return out
