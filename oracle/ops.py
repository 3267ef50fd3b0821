"""CPU oracle for the relational-GNN hot path -- TEST INFRASTRUCTURE ONLY.

A plain-PyTorch restatement (torch's own index / matmul ops, none of this repo's kernels; fp32 or fp64; evaluated on
the CPU by the small tests and -- it is device-agnostic -- in fp64 on the GPU by the full-size checks of
tests/test_gpu_fullsize.py, where the CPU would take minutes) of what each
``torch.ops.torch_hrt.*`` op on the hot path computes, one function per op,
with the reference's argument order and its in-place, caller-allocated-output
convention.  Only ``tests/``, ``__graft_entry__.smoke()`` and ``bench.py``'s
``cpu_baseline`` leg may import this module; the product (``het_amd``) never
does.

PARITY STATUS: the reference's CUDA path cannot be built
or run here (no nvcc, empty third_party/ submodules) and the reference ships no
arithmetic test vectors, so for the floating-point ops this restatement follows
the CUDA sources as text (file:line cited per function) and is "parity
unpinned", except:
  * layouts (integer, exact);
  * the ``exp`` / ``sum`` outputs of the fused GAT forward (a4), CompactAsOfNodeKind 0 and 4
    (ref_rgat.py:5-32 and its dual-unique-list wrapper :77-115);
  * ``grad_feat_src`` of the fused GAT backward (a5; ref_rgat.py:66-75), CompactAsOfNodeKind 0;
  * round 5: a4 ``exp`` / ``sum`` for kind 1 (the same wrapper fed the two-sided unique list) and ``sum`` for kind 2
    (ref_rgat.py:182-220, one inverse index for both edge ends; that wrapper loses its ``exp``), and a5 ``grad_feat`` for
    kinds 4 and 1 (ref_rgat.py:66-75 on the exp / sum of the compact forwards; compact rows summed per source node)
    are pinned by golden vectors generated from the reference's own importable Python
    (tests/golden/make_golden.py; tests/test_oracle.py::*_golden, tests/test_gpu_ops.py::test_gat_golden_*,
    tests/test_mag01_full.py, tests/test_gpu_mag01_full.py; toy graph, slice and the whole shipped topology).
    Pinned by the reference: a4 forward kinds 0 / 1 / 2 (sum) / 4, a5 ``grad_feat`` kinds 0 / 1 / 4.  Kind 3 is kind 4 with the
    rows found by search instead of read from the inverse index (same rows: tests/test_oracle.py::test_gat_kind3_rows_equal_kind4).
  * a9 (RGCN compact aggregation) forward and backward (ref_rgcn.py:63-100), the KEYING of a10's softmax (ref_hgt.py:78-136,
    :269-296: denominator per destination over all E positions, relation -> mu row; not its exp and sum) and a10c's message
    aggregation and its backward (ref_hgt.py:299-337): tests/golden/*_rgcn_hgt.npz, tests/test_rgcn_hgt_golden.py,
    tests/test_gpu_rgcn_hgt_golden.py (DESIGN.md section 3 states what each vector does and does not pin).
    NOT pinned, because the reference holds nothing comparable: a4's ``ret`` (ref_rgat.py never writes it), a5's
    ``grad_el`` / ``grad_er`` (ref_rgat.py:64-65 adds ``slope`` to the leaky-ReLU derivative and drops the dot product
    over the feature dimension -- it disagrees with the CUDA kernel it mirrors; its two backward WRAPPERS, :117-180 and
    :222-270, raise a RuntimeError for every shape -- run as written by make_golden.py), and every other floating-point op.
Where the CUDA code deviates from the reference's own stated intent (its DSL
specs hrt/pyctor/examples/inter-op-dsl/*.inter-op and in-code TODO/FIXMEs) the
oracle implements the INTENDED semantics; each such position is listed in
DESIGN.md ("Reference quirks") with its SURVEY.md section-9 id.  The ops with a deterministic
quirk (Q3, Q4, Q6, Q7) also take ``reference_literal=True``: what the CUDA code computes as written,
index for index, so that the distance between the two readings can be measured
(tests/test_oracle.py::test_reference_literal_distance_on_the_shipped_topology).
Nothing in het_amd implements the literal readings.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

Tensor = torch.Tensor


# --------------------------------------------------------------------------
# helpers
# --------------------------------------------------------------------------
def rel_of_position(rel_ptrs: Tensor) -> Tensor:
    """Relation id of every position of a relation-bucketed list (the device
    code recovers it by searching ``rel_ptrs``: hrt/include/utils.cu.h:94-121)."""
    R = rel_ptrs.numel() - 1
    return torch.repeat_interleave(torch.arange(R, dtype=torch.int64, device=rel_ptrs.device), rel_ptrs[1:] - rel_ptrs[:-1])


def _search_rows(rel_ptrs_u: Tensor, nodes_u: Tensor, rel: Tensor, node: Tensor, num_nodes_bound: int) -> Tensor:
    """Row of (rel, node) in a per-relation sorted unique list
    (``find_relational_compact_as_of_node_index`` with binary search,
    hrt/include/kernel_enums.h:101-119)."""
    key_u = rel_of_position(rel_ptrs_u) * num_nodes_bound + nodes_u
    key = rel * num_nodes_bound + node
    pos = torch.searchsorted(key_u, key)
    assert bool((key_u[pos] == key).all()), "(relation, node) pair missing from the unique list"
    return pos


def _gat_rows(kind: int, d: Dict[str, Tensor], rel_ptrs, row, col, eids):
    """(src_row, dst_row): rows of feat/el (src side) and er (dst side) for each
    edge position.  RGATKernelsSeparateCOO.cu.h:139-189 and kernel_enums.h."""
    if kind == 0:
        return eids, eids
    rel = rel_of_position(rel_ptrs)
    bound = int(max(row.max(), col.max())) + 1 if row.numel() else 1
    if kind == 1:  # Enabled: one two-sided unique list, binary search
        rp, nodes = d["unique_srcs_and_dests_rel_ptrs"], d["unique_srcs_and_dests_node_indices"]
        return _search_rows(rp, nodes, rel, row, bound), _search_rows(rp, nodes, rel, col, bound)
    if kind == 3:  # EnabledWithDualList: separate src / dst unique lists
        rp_c = d.get("unique_srcs_and_dests_rel_ptrs_col", d.get("unique_srcs_and_dests_rel_col"))
        return (
            _search_rows(d["unique_srcs_and_dests_rel_ptrs"], d["unique_srcs_and_dests_node_indices_row"], rel, row, bound),
            _search_rows(rp_c, d["unique_srcs_and_dests_node_indices_col"], rel, col, bound),
        )
    if kind == 4:  # EnabledWithDualListWithDirectIndexing: inverse index by edata idx
        return d["edata_idx_to_inverse_idx_row"][eids], d["edata_idx_to_inverse_idx_col"][eids]
    if kind == 2:  # EnabledWithDirectIndexing: the reference hands ONE mapper to both lookups and direct indexing ignores
        # the node id (RGATKernelsSeparateCOO.cu.h:163-170, kernel_enums.h:117): both rows are that index of the edge
        m = d["edata_idx_to_inverse_idx"][eids]
        return m, m
    raise NotImplementedError(f"CompactAsOfNodeKind {kind}")


# --------------------------------------------------------------------------
# a1/a2  segment GEMM with gather / scatter lists
# --------------------------------------------------------------------------
def _matmul_lists(d: Dict[str, Tensor], kind: int):
    if kind == 0:
        return d["separate_coo_rel_ptrs"], d["separate_coo_node_indices"], d["separate_coo_eids"]
    if kind == 1:
        rp = d["unique_srcs_and_dests_rel_ptrs"]
        return rp, d["unique_srcs_and_dests_node_indices"], torch.arange(int(rp[-1]), dtype=torch.int64, device=rp.device)
    raise NotImplementedError(f"CompactAsOfNodeKind {kind} (the reference asserts, RGNNOps.inc.h:292-294)")


def rgnn_relational_matmul(d, kind: int, W: Tensor, x: Tensor, ret: Tensor, in1head: bool) -> None:
    """ret[scatter[i], h, :] = x[gather[i], (h), :] @ W[rel(i), h]   (plain store)

    RGNNOps.inc.h:238-295 -> _RelationalMatMul :93-236 ->
    my_shmem_sgemm_func.cu.h:504-531 (kind 0), :635-664 (gather == scatter),
    :671-704 (kind 1: gather by the unique (rel, node) list, dense output rows).
    Per-head semantics for in1head == False are the intended ones."""
    rp, g, s = _matmul_lists(d, kind)
    R, H, K, D = W.shape
    retv = ret.view(-1, H, D)
    for r in range(R):
        a, b = int(rp[r]), int(rp[r + 1])
        if a == b:
            continue
        xin = x.reshape(x.shape[0], -1)[g[a:b]]
        if in1head:
            out = torch.einsum("nk,hkd->nhd", xin.view(-1, K), W[r])
        else:
            out = torch.einsum("nhk,hkd->nhd", xin.view(-1, H, K), W[r])
        retv[s[a:b]] = out


def backward_rgnn_relational_matmul(d, kind: int, Wt: Tensor, x: Tensor, gradout: Tensor,
                                    grad_x: Tensor, grad_W: Tensor, in1head: bool) -> None:
    """grad_x[gather[i]] += sum_h gradout[scatter[i], h] @ Wt[r, h]   (heads summed iff in1head)
    grad_W[r, h]      += x[gather[i], (h)]^T (x) gradout[scatter[i], h]

    RGNNOps.inc.h:946-1010 -> :756-944; kernels my_shmem_sgemm_func.cu.h:711-776.
    Wt is W with its last two dims transposed ([R, H, D, K])."""
    rp, g, s = _matmul_lists(d, kind)
    R, H, D, K = Wt.shape
    go = gradout.reshape(-1, H, D)
    gx = grad_x.view(grad_x.shape[0], -1)
    for r in range(R):
        a, b = int(rp[r]), int(rp[r + 1])
        if a == b:
            continue
        gr = go[s[a:b]]
        xin = x.reshape(x.shape[0], -1)[g[a:b]]
        if in1head:
            gx.index_add_(0, g[a:b], torch.einsum("nhd,hdk->nk", gr, Wt[r]))
            grad_W[r] += torch.einsum("nk,nhd->hkd", xin.view(-1, K), gr)
        else:
            gx.index_add_(0, g[a:b], torch.einsum("nhd,hdk->nhk", gr, Wt[r]).reshape(b - a, H * K))
            grad_W[r] += torch.einsum("nhk,nhd->hkd", xin.view(-1, H, K), gr)


# --------------------------------------------------------------------------
# a3  contiguous-segment GEMM
# --------------------------------------------------------------------------
def rgnn_relational_matmul_no_scatter_gather_list(offsets: Tensor, W: Tensor, x: Tensor, ret: Tensor) -> None:
    """Rows offsets[t]:offsets[t+1] use W[t]:  ret[i, h, :] = x[i, (h), :] @ W[t, h].
    x is [rows, K] (one head shared by all weight heads) or [rows, H, K].
    RGNNOps.inc.h:21-88; kernel my_shmem_sgemm_func.cu.h:538-564."""
    T, H, K, D = W.shape
    n = x.shape[0]
    per_head = x.numel() == n * H * K and H > 1
    retv = ret.view(n, H, D)
    for t in range(T):
        a, b = int(offsets[t]), int(offsets[t + 1])
        if a == b:
            continue
        if per_head:
            retv[a:b] = torch.einsum("nhk,hkd->nhd", x[a:b].reshape(-1, H, K), W[t])
        else:
            retv[a:b] = torch.einsum("nk,hkd->nhd", x[a:b].reshape(-1, K), W[t])


def backward_rgnn_relational_matmul_no_scatter_gather_list(offsets: Tensor, Wt: Tensor, x: Tensor, gradout: Tensor,
                                                            grad_x: Tensor, grad_W: Tensor) -> None:
    """RGNNOps.inc.h:660-753; kernels my_shmem_sgemm_func.cu.h:571-628."""
    T, H, D, K = Wt.shape
    n = x.shape[0]
    per_head = x.numel() == n * H * K and H > 1
    go = gradout.reshape(n, H, D)
    for t in range(T):
        a, b = int(offsets[t]), int(offsets[t + 1])
        if a == b:
            continue
        if per_head:
            grad_x.view(n, H, K)[a:b] += torch.einsum("nhd,hdk->nhk", go[a:b], Wt[t])
            grad_W[t] += torch.einsum("nhk,nhd->hkd", x[a:b].reshape(-1, H, K), go[a:b])
        else:
            grad_x.view(n, K)[a:b] += torch.einsum("nhd,hdk->nk", go[a:b], Wt[t])
            grad_W[t] += torch.einsum("nk,nhd->hkd", x[a:b].reshape(-1, K), go[a:b])


# --------------------------------------------------------------------------
# a4/a5  fused GAT: edge softmax over all in-edges of a destination + aggregation
# --------------------------------------------------------------------------
def _leaky_exp(z: Tensor, slope: float) -> Tensor:
    # gatLeakyReluExp, GAT/FusedGAT.cu.h:23-26: val > 0 ? exp(val) : exp(slope * val)
    return torch.exp(torch.where(z > 0, z, z * slope))


def relational_fused_gat_separate_coo(eids, rel_ptrs, row, col, kind: int, d, feat, el, er,
                                      sum_, exp, ret, slope: float) -> None:
    """exp[eid, h]   = leaky_exp(el[srow, h] + er[drow, h])
    sum[dst, h]   = SUM over ALL in-edges of dst (every relation) of exp   (no max-subtraction)
    ret[dst,h,:]  = SUM exp[eid,h] / sum[dst,h] * feat[srow, h, :]

    RGATOps.inc.h:170-245 -> :19-167; kernels RGAT/RGATKernelsSeparateCOO.cu.h:117-204
    (exp + sum) and :17-100 (aggregation).  ``sum`` and ``ret`` are zeroed here: the
    reference accumulates into ``new_empty`` buffers."""
    H = el.shape[1]
    srow, drow = _gat_rows(kind, d, rel_ptrs, row, col, eids)
    e = _leaky_exp(el.reshape(el.shape[0], H)[srow] + er.reshape(er.shape[0], H)[drow], slope)  # [E, H] by position
    exp.view(-1, H)[eids] = e
    sum_.zero_()
    sum_.view(-1, H).index_add_(0, col, e)
    a = e / sum_.view(-1, H)[col]
    ret.zero_()
    N = ret.shape[0]
    ret.view(N, H, -1).index_add_(0, col, a.unsqueeze(-1) * feat.reshape(feat.shape[0], H, -1)[srow])


def backward_relational_fused_gat_separate_coo(eids, rel_ptrs, row, col, kind: int, d, feat, el, er,
                                               sum_, exp, ret, gradout, grad_feat, grad_el, grad_er,
                                               slope: float) -> None:
    """a = exp[eid,h] / sum[dst,h]
    grad_feat[srow,h,:] += a * gradout[dst,h,:]
    t = SUM_d gradout[dst,h,d] * (feat[srow,h,d] - ret[dst,h,d]) * a * (z > 0 ? 1 : slope),  z = el[srow,h]+er[drow,h]
    grad_el[srow,h] += t ;  grad_er[drow,h] += t

    RGATOps.inc.h:465-551; kernel RGAT/RGATBackwardKernelsSeparateCOO.cu.h:9-117
    (gradLeaky: GAT/FusedGATBackward.cu.h)."""
    H = el.shape[1]
    N = ret.shape[0]
    srow, drow = _gat_rows(kind, d, rel_ptrs, row, col, eids)
    a = exp.view(-1, H)[eids] / sum_.view(-1, H)[col]  # [E, H]
    go = gradout.reshape(N, H, -1)[col]  # [E, H, D]
    f = feat.reshape(feat.shape[0], H, -1)
    grad_feat.view(feat.shape[0], H, -1).index_add_(0, srow, a.unsqueeze(-1) * go)
    z = el.reshape(el.shape[0], H)[srow] + er.reshape(er.shape[0], H)[drow]
    dleaky = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))
    t = (go * (f[srow] - ret.view(N, H, -1)[col])).sum(-1) * a * dleaky
    grad_el.view(-1, H).index_add_(0, srow, t)
    grad_er.view(-1, H).index_add_(0, drow, t)


def relational_fused_gat_csr(in_row_ptrs, in_col, in_eids, in_reltypes, uniq_rel_ptrs, uniq_node_idx,
                             feat, el, er, sum_, exp, ret, slope: float, compact: bool = False) -> None:
    """Vertex-parallel twin over the in-CSR (rows = dst, col_indices = src):
    same math as the separate-COO op.  RGATOps.inc.h:251-277; kernels
    GAT/FusedGAT.cu.h:107-116, 213-222."""
    N = in_row_ptrs.numel() - 1
    dst = torch.repeat_interleave(torch.arange(N, dtype=torch.int64, device=in_row_ptrs.device), in_row_ptrs[1:] - in_row_ptrs[:-1])
    H = el.shape[1]
    if compact:
        bound = N
        srow = _search_rows(uniq_rel_ptrs, uniq_node_idx, in_reltypes, in_col, bound)
        drow = _search_rows(uniq_rel_ptrs, uniq_node_idx, in_reltypes, dst, bound)
    else:
        srow = drow = in_eids
    e = _leaky_exp(el.reshape(el.shape[0], H)[srow] + er.reshape(er.shape[0], H)[drow], slope)
    exp.view(-1, H)[in_eids] = e
    sum_.zero_()
    sum_.view(-1, H).index_add_(0, dst, e)
    ret.zero_()
    ret.view(N, H, -1).index_add_(0, dst, (e / sum_.view(-1, H)[dst]).unsqueeze(-1) * feat.reshape(feat.shape[0], H, -1)[srow])


def backward_relational_fused_gat_csr(out_row_ptrs, out_col, out_eids, out_reltypes, uniq_rel_ptrs, uniq_node_idx,
                                      feat, el, er, sum_, exp, ret, gradout, grad_feat, grad_el, grad_er,
                                      slope: float, compact: bool = False) -> None:
    """Backward over the out-CSR (rows = src, col_indices = dst).
    RGATOps.inc.h:430-460; kernels GAT/FusedGATBackward.cu.h:138-362."""
    N = out_row_ptrs.numel() - 1
    src = torch.repeat_interleave(torch.arange(N, dtype=torch.int64, device=out_row_ptrs.device), out_row_ptrs[1:] - out_row_ptrs[:-1])
    dst = out_col
    H = el.shape[1]
    if compact:
        srow = _search_rows(uniq_rel_ptrs, uniq_node_idx, out_reltypes, src, N)
        drow = _search_rows(uniq_rel_ptrs, uniq_node_idx, out_reltypes, dst, N)
    else:
        srow = drow = out_eids
    a = exp.view(-1, H)[out_eids] / sum_.view(-1, H)[dst]
    go = gradout.reshape(N, H, -1)[dst]
    f = feat.reshape(feat.shape[0], H, -1)
    grad_feat.view(feat.shape[0], H, -1).index_add_(0, srow, a.unsqueeze(-1) * go)
    z = el.reshape(el.shape[0], H)[srow] + er.reshape(er.shape[0], H)[drow]
    dleaky = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))
    t = (go * (f[srow] - ret.view(N, H, -1)[dst])).sum(-1) * a * dleaky
    grad_el.view(-1, H).index_add_(0, srow, t)
    grad_er.view(-1, H).index_add_(0, drow, t)


# --------------------------------------------------------------------------
# a7/a8  fused RGCN layer
# --------------------------------------------------------------------------
def rgcn_layer1_separate_coo(rel_ptrs, eids, row, col, x, W, norm, ret) -> None:
    """ret[col[i], :] += (x[row[i], :] * norm[eids[i]]) @ W[rel(i)]
    RGCNOps.inc.h:84-138; kernel my_shmem_sgemm_func_rgcn_hgt.cu.h:597-625.
    ``ret`` is accumulated into (Python zero-fills it, rgcn_layers_and_funcs.py:578-583)."""
    R = W.shape[0]
    nv = norm.reshape(-1)
    for r in range(R):
        a, b = int(rel_ptrs[r]), int(rel_ptrs[r + 1])
        if a == b:
            continue
        msg = (x[row[a:b]] * nv[eids[a:b]].unsqueeze(-1)) @ W[r]
        ret.index_add_(0, col[a:b], msg)


def backward_rgcn_layer1_separate_coo(rel_ptrs, eids, row, col, x, Wt, norm, grad_norm, grad_x, gradout, grad_W,
                                      reference_literal: bool = False) -> None:
    """grad_x[row[i]] += (gradout[col[i]] * norm[eids[i]]) @ Wt[r]       (intended direction, SURVEY Q3:
                        the CUDA code gathers gradout by row and scatters to col)
    grad_W[r]       += (x[row[i]] * norm[eids[i]])^T (x) gradout[col[i]]
    grad_norm is left untouched (the reference disables that output,
    my_shmem_sgemm_func_rgcn_hgt.cu.h:680-684).  RGCNOps.inc.h:368-467.
    reference_literal: grad_x[col[i]] += (gradout[row[i]] * norm[eids[i]]) @ Wt[r] -- the kernel's A_gather_list is
    separate_coo_row_idx and its C_scatter_list separate_coo_col_idx in the non-outer-product case
    (my_shmem_sgemm_func_rgcn_hgt.cu.h:118-125, launched for this op at :680-698 with the forward's COO); grad_W as above
    (outer-product case: A by row, B by col -- correct as coded)."""
    R = Wt.shape[0]
    nv = norm.reshape(-1)
    for r in range(R):
        a, b = int(rel_ptrs[r]), int(rel_ptrs[r + 1])
        if a == b:
            continue
        sc = nv[eids[a:b]].unsqueeze(-1)
        g = gradout[col[a:b]] * sc
        if reference_literal:
            grad_x.index_add_(0, col[a:b], (gradout[row[a:b]] * sc) @ Wt[r])
        else:
            grad_x.index_add_(0, row[a:b], g @ Wt[r])
        grad_W[r] += (x[row[a:b]]).t() @ g


# --------------------------------------------------------------------------
# a9  RGCN aggregation of a compact (relation, src) feature tensor
# --------------------------------------------------------------------------
def _rgcn_compact_rows(d, direct: bool, rel_ptrs, row, eids):
    if direct:
        return d["inverse_indices_row"][eids]
    bound = int(row.max()) + 1 if row.numel() else 1
    return _search_rows(d["rel_ptrs_row"], d["node_indices_row"], rel_of_position(rel_ptrs), row, bound)


def rgcn_node_mean_aggregation_compact_as_of_node_separate_coo(eids, rel_ptrs, row, col, d, feat, enorm, ret,
                                                               direct: bool, reference_literal: bool = False) -> None:
    """ret[col[i], :] += enorm[eids[i]] * feat[compact_row(rel(i), row[i]), :]
    RGCNOps.inc.h:24-82; kernel RGCN/RGCNKernelsEdgeParallel.cu.h:20-92 (which indexes feat by
    the raw src id -- its own TODO; intended mapping used here).  ``ret`` zeroed
    here (allocated with th.empty by the caller, rgcn_layers_and_funcs.py:763-768).
    reference_literal: feat row = row[i], the raw source id (RGCNKernelsEdgeParallel.cu.h:53-56 ``feat_src_entry_id =
    src_vid``) -- defined only while every source id is below the number of compact rows (it reads out of bounds otherwise;
    refused here)."""
    if reference_literal:
        assert not row.numel() or int(row.max()) < feat.shape[0], "the literal reading indexes the compact tensor out of bounds here"
        fr = row
    else:
        fr = _rgcn_compact_rows(d, direct, rel_ptrs, row, eids)
    ret.zero_()
    ret.view(ret.shape[0], -1).index_add_(0, col, enorm.reshape(-1)[eids].unsqueeze(-1) * feat.reshape(feat.shape[0], -1)[fr])


def backward_rgcn_node_mean_aggregation_compact_as_of_node_separate_coo(eids, rel_ptrs, row, col, d, feat, enorm, ret,
                                                                        gradout, grad_feat, direct: bool) -> None:
    """grad_feat[compact_row, :] += enorm[eids[i]] * gradout[col[i], :]
    RGCNOps.inc.h:303-366; kernel RGCN/RGCNBackwardKernelsEdgeParallel.cu.h:21-92."""
    fr = _rgcn_compact_rows(d, direct, rel_ptrs, row, eids)
    grad_feat.view(grad_feat.shape[0], -1).index_add_(
        0, fr, enorm.reshape(-1)[eids].unsqueeze(-1) * gradout.reshape(gradout.shape[0], -1)[col])


# --------------------------------------------------------------------------
# a12  edge-wise inner product  <left[lrow(i)], right[row[i]]>   (HGT attention score, unfused path)
# --------------------------------------------------------------------------
def _left_rows(d, kind: int, rel_ptrs, col, eids):
    if kind == 0:
        return eids
    if kind == 1:  # compact left operand: row of (relation, col[i]) in the "_col" unique list
        bound = int(max(int(col.max()), int(d["unique_srcs_and_dests_node_indices"].max()))) + 1 if col.numel() else 1
        return _search_rows(d["unique_srcs_and_dests_rel_ptrs"], d["unique_srcs_and_dests_node_indices"],
                            rel_of_position(rel_ptrs), col, bound)
    if kind == 2:
        return d["edata_idx_to_inverse_idx"][eids]
    raise NotImplementedError(kind)


def rgnn_inner_product_right_node_separatecoo(d, kind: int, rel_ptrs, eids, row, col, left, right, out) -> None:
    """out[eids[i], h] = < left[lrow(i), h, :], right[row[i], h, :] >      (out overwritten)
    lrow(i) = eids[i] (kind 0) | row of (rel(i), col[i]) in the unique list (kind 1) | inverse index (kind 2).
    RGNNOps.inc.h:609-658 -> :296-440; kernel RGNN/InnerProductEdgeParallel.cu.h:13-113 (which names
    the row index "dst"; the HGT layer passes left = q[dst].W_att per edge / per (rel, dst) and
    right = k, hrt/python/HGT/models.py:217-241)."""
    H = out.shape[1]
    lr = _left_rows(d, kind, rel_ptrs, col, eids)
    l = left.reshape(left.shape[0], H, -1)[lr]
    r = right.reshape(right.shape[0], H, -1)[row]
    out.view(-1, H)[eids] = (l * r).sum(-1)


def backward_inner_product_right_node_separatecoo(d, kind: int, rel_ptrs, eids, row, col, left, right, gradout,
                                                  grad_left, grad_right) -> None:
    """grad_left[lrow(i), h, :] += gradout[eids[i], h] * right[row[i], h, :]
    grad_right[row[i], h, :]  += gradout[eids[i], h] * left[lrow(i), h, :]
    Accumulating (the CUDA kernel stores without atomics and mixes up row/col, SURVEY Q8:
    RGNN/InnerProductEdgeParallel.cu.h:119-202).  RGNNOps.inc.h:1131-1181."""
    H = gradout.shape[1]
    lr = _left_rows(d, kind, rel_ptrs, col, eids)
    g = gradout.reshape(-1, H)[eids].unsqueeze(-1)
    grad_left.view(grad_left.shape[0], H, -1).index_add_(0, lr, g * right.reshape(right.shape[0], H, -1)[row])
    grad_right.view(grad_right.shape[0], H, -1).index_add_(0, row, g * left.reshape(left.shape[0], H, -1)[lr])


# --------------------------------------------------------------------------
# a10  HGT edge softmax with per-relation temperature mu
# --------------------------------------------------------------------------
def hgt_full_graph_edge_softmax_ops_separate_coo(row, col, eids, rel_ptrs, score, mu, sum_, m, a,
                                                 reference_literal: bool = False) -> None:
    """m[eid,h] = exp(score[eid,h] * mu[r,h]);  sum[dst,h] = SUM over in-edges of dst;  a = m / sum[dst].
    Denominator keyed by the DESTINATION (col) over all E edges -- the intended semantics (the CUDA code
    keys by row_indices and drops the last edge).  HGTOpsEdgeParallel.inc.h:18-31 ->
    HGTOps.inc.h:23-106; kernels HGT/HGTForwardKernels.cu.h:594-761.
    reference_literal: the launcher passes ``numel() - 1`` of the row-index array as the edge count (HGTOps.inc.h:70-71: the
    argument doubles as a CSR row-pointer array in the vertex-parallel twin), so the LAST position is never visited (its m and a
    keep what the caller's buffers held), and both kernels key the denominator by ``row_indices`` (HGTForwardKernels.cu.h:619
    accumulates into sum[row[i]], :722 divides by it): a softmax over the OUT-edges of the source.  ``sum`` is accumulated into
    as given (no fill in the launcher)."""
    H = score.shape[1]
    rel = rel_of_position(rel_ptrs)
    if reference_literal:
        n = max(0, eids.numel() - 1)
        e, r_, key = eids[:n], rel[:n], row[:n]
        mm = torch.exp(score.reshape(-1, H)[e] * mu.reshape(-1, H)[r_])
        m.view(-1, H)[e] = mm
        sum_.view(-1, H).index_add_(0, key, mm)
        a.view(-1, H)[e] = mm / sum_.view(-1, H)[key]
        return
    mm = torch.exp(score.reshape(-1, H)[eids] * mu.reshape(-1, H)[rel])
    m.view(-1, H)[eids] = mm
    sum_.zero_()
    sum_.view(-1, H).index_add_(0, col, mm)
    a.view(-1, H)[eids] = mm / sum_.view(-1, H)[col]


def backward_hgt_full_graph_enorm_to_unnormalized_attn_score_separate_coo(row, col, eids, rel_ptrs, score, a, grad_a,
                                                                          mu, grad_score, grad_mu, tmp,
                                                                          reference_literal: bool = False) -> None:
    """tmp[dst,h] = SUM_in-edges a*grad_a;  c = (grad_a - tmp[dst]) * a;
    grad_score[eid,h] = c * mu[r,h];  grad_mu[r,h] += SUM c * score[eid,h].
    Intended formulas from the kernel's own comments (HGT/HGTBackwardKernels.cu.h:161-168, 309-312;
    the code omits '* score' and loops over a fraction of the edges).  HGTOps.inc.h:597-648.
    reference_literal: the kernel is launched on the type-1 schedule (ThreadingGridsBlocksSchedules.h:9-26: threads (1, 32),
    blocks (H, G), G = min(ceil(E / 32), 65535)) but its loops start at ``threadIdx`` alone (HGTBackwardKernels.cu.h:270 ``e =
    threadIdx.y; e += blockDim.y * gridDim.y``, :290 ``head_idx = threadIdx.x; += blockDim.x * gridDim.x``): every one of the
    H * G blocks visits the SAME positions e = t + 32 G k (t < 32) and head 0 only.  Stage 0 therefore adds grad_a * a of those
    (position, head 0) pairs H * G times into tmp[row[e], 0] (keyed by the source, :304); stage 1 stores grad_score[eid, 0] =
    (grad_a - tmp[row[e], 0]) * a * mu (idempotent) and adds (grad_a - tmp) * a -- without ``* score``, :325-329 -- H * G times
    into grad_mu[r, 0].  Every other (edge, head) of grad_score keeps what the caller's buffer held; tmp and grad_mu are
    accumulated into as given."""
    H = score.shape[1]
    rel = rel_of_position(rel_ptrs)
    if reference_literal:
        E = eids.numel()
        G = min((E + 31) // 32, 65535)
        pos = torch.arange(E)
        pos = pos[(pos % (32 * G)) < 32] if G else pos[:0]
        e, r_, key = eids[pos], rel[pos], row[pos]
        av, gv = a.reshape(-1, H)[e, 0], grad_a.reshape(-1, H)[e, 0]
        times = float(H * G)
        tmp.view(-1, H)[:, 0].index_add_(0, key, times * av * gv)
        c = (gv - tmp.view(-1, H)[key, 0]) * av
        grad_score.view(-1, H)[e, 0] = c * mu.reshape(-1, H)[r_, 0]
        grad_mu.view(-1, H)[:, 0].index_add_(0, r_, times * c)
        return
    av, gv = a.reshape(-1, H)[eids], grad_a.reshape(-1, H)[eids]
    tmp.zero_()
    tmp.view(-1, H).index_add_(0, col, av * gv)
    c = (gv - tmp.view(-1, H)[col]) * av
    grad_score.view(-1, H)[eids] = c * mu.reshape(-1, H)[rel]
    grad_mu.view(-1, H).index_add_(0, rel, c * score.reshape(-1, H)[eids])


# --------------------------------------------------------------------------
# a11  HGT fused message generation + attention-weighted aggregation
# --------------------------------------------------------------------------
def hgt_full_graph_fused_message_calc_and_mean_aggregation_separate_coo(rel_ptrs, eids, row, col, v, W, a, new_h) -> None:
    """new_h[col[i], h, :] += (v[row[i], h, :] * a[eids[i], h]) @ W[r, h]        (new_h zero-filled by the caller,
    hgt_layers_and_funcs.py:462-469).  HGTOpsEdgeParallel.inc.h:33-88; kernel
    my_shmem_sgemm_func_rgcn_hgt.cu.h:708-740."""
    R, H, dk, do = W.shape
    N = new_h.shape[0]
    for r in range(R):
        a0, b0 = int(rel_ptrs[r]), int(rel_ptrs[r + 1])
        if a0 == b0:
            continue
        msg = torch.einsum("nhk,hkd->nhd", v.reshape(v.shape[0], H, dk)[row[a0:b0]] * a.reshape(-1, H)[eids[a0:b0]].unsqueeze(-1), W[r])
        new_h.view(N, H, do).index_add_(0, col[a0:b0], msg)


def backward_hgt_full_graph_fused_message_calc_and_mean_aggregation_separate_coo(rel_ptrs, eids, row, col, v, Wt, a,
                                                                                 new_h, grad_v, grad_W, grad_a,
                                                                                 gradout, reference_literal: bool = False) -> None:
    """grad_v[row[i],h,:] += (gradout[col[i],h,:] * a) @ Wt[r,h]      (intended direction, same quirk as SURVEY Q3)
    grad_W[r,h]        += (v[row[i],h,:] * a)^T (x) gradout[col[i],h,:]
    grad_a[eids[i],h]   = < gradout[col[i],h,:] @ Wt[r,h], v[row[i],h,:] >
    HGTOpsEdgeParallel.inc.h:295-369; kernels my_shmem_sgemm_func_rgcn_hgt.cu.h:747-816.
    reference_literal (Q3 on this op): the input-gradient kernel (:780-816) gathers A = gradout by ``row`` scaled by a
    (:391-400), scatters C to ``col`` (:118-125) and takes its inner-product term from v at the C row (:230-237):
    grad_v[col[i],h,:] += (gradout[row[i],h,:] * a) @ Wt[r,h];  grad_a[eids[i],h] += < (gradout[row[i],h,:] * a) @ Wt[r,h],
    v[col[i],h,:] > (atomicAdd into the caller's buffer, :577).  grad_W as above."""
    R, H, do, dk = Wt.shape
    N = gradout.shape[0]
    for r in range(R):
        a0, b0 = int(rel_ptrs[r]), int(rel_ptrs[r + 1])
        if a0 == b0:
            continue
        av = a.reshape(-1, H)[eids[a0:b0]].unsqueeze(-1)
        go = gradout.reshape(N, H, do)[col[a0:b0]]
        vv = v.reshape(v.shape[0], H, dk)[row[a0:b0]]
        if reference_literal:
            back_l = torch.einsum("nhd,hdk->nhk", gradout.reshape(N, H, do)[row[a0:b0]] * av, Wt[r])
            grad_v.view(v.shape[0], H, dk).index_add_(0, col[a0:b0], back_l)
            grad_W[r] += torch.einsum("nhk,nhd->hkd", vv * av, go)
            grad_a.view(-1, H).index_add_(0, eids[a0:b0], (back_l * v.reshape(v.shape[0], H, dk)[col[a0:b0]]).sum(-1))
            continue
        back = torch.einsum("nhd,hdk->nhk", go, Wt[r])
        grad_v.view(v.shape[0], H, dk).index_add_(0, row[a0:b0], back * av)
        grad_W[r] += torch.einsum("nhk,nhd->hkd", vv * av, go)
        grad_a.view(-1, H)[eids[a0:b0]] = (back * vv).sum(-1)


# --------------------------------------------------------------------------
# HGT fused attention score (alternative to a1 + a12)
# --------------------------------------------------------------------------
def hgt_full_graph_hetero_attention_ops_coo(row, col, eids, rel_ptrs, k, q, W, inner, score) -> None:
    """inner[eid,h,:] = k[row[i],h,:] @ W[r,h];  score[eid,h] = < inner[eid,h,:], q[col[i],h,:] >.
    HGTOpsEdgeParallel.inc.h:95-158; kernel my_shmem_sgemm_func_rgcn_hgt.cu.h:823-857."""
    R, H, dk, do = W.shape
    for r in range(R):
        a0, b0 = int(rel_ptrs[r]), int(rel_ptrs[r + 1])
        if a0 == b0:
            continue
        inn = torch.einsum("nhk,hkd->nhd", k.reshape(k.shape[0], H, dk)[row[a0:b0]], W[r])
        inner.view(-1, H, do)[eids[a0:b0]] = inn
        score.view(-1, H)[eids[a0:b0]] = (inn * q.reshape(q.shape[0], H, do)[col[a0:b0]]).sum(-1)


def backward_hgt_full_graph_hetero_attention_ops_coo(in_row_ptrs, in_col, in_eids, in_reltypes, row, col, eids, rel_ptrs,
                                                     grad_W, Wt, k, q, inner, grad_score, grad_k, grad_q) -> None:
    """grad_q[col[i],h,:] += gs * inner[eid,h,:];  grad_k[row[i],h,:] += gs * (q[col[i],h,:] @ Wt[r,h]);
    grad_W[r,h] += k[row[i],h,:]^T (x) (gs * q[col[i],h,:]),   gs = grad_score[eid,h].
    HGTOpsEdgeParallel.inc.h:166-293 (the in-CSR arguments feed its vertex-parallel dq kernel; unused here)."""
    R, H, do, dk = Wt.shape
    for r in range(R):
        a0, b0 = int(rel_ptrs[r]), int(rel_ptrs[r + 1])
        if a0 == b0:
            continue
        gs = grad_score.reshape(-1, H)[eids[a0:b0]].unsqueeze(-1)
        qq = q.reshape(q.shape[0], H, do)[col[a0:b0]]
        kk = k.reshape(k.shape[0], H, dk)[row[a0:b0]]
        grad_q.view(q.shape[0], H, do).index_add_(0, col[a0:b0], gs * inner.reshape(-1, H, do)[eids[a0:b0]])
        grad_k.view(k.shape[0], H, dk).index_add_(0, row[a0:b0], torch.einsum("nhd,hdk->nhk", gs * qq, Wt[r]))
        grad_W[r] += torch.einsum("nhk,nhd->hkd", kk, gs * qq)


# --------------------------------------------------------------------------
# HGT attention + aggregation on the distinct (relation, source) rows (no reference op of its own: the chain
# relation_att product -> inner product -> edge softmax -> message product + aggregation of HGT/models.py:172-262 with its
# source side pre-multiplied per (relation, source) row; include/het_amd.h het_hgt_aggregate_compact)
# --------------------------------------------------------------------------
def hgt_attention_rows(kv_c, q, srow, col, num_nodes):
    """kv_c [S_row, 2, H, D] (k' then m of every (relation, source) row), q [N, H, D], srow / col [E]: the row and the
    destination of every edge.  Returns (lsum [N,H], out [N,H,D]); differentiable (autograd gives the backward op's outputs).
    exp without a running maximum, softmax over ALL in-edges of a destination (layers.hgt_layer)."""
    H = q.shape[1]
    s = (kv_c[srow, 0] * q[col]).sum(-1)
    w = torch.exp(s)
    lsum = torch.zeros(num_nodes, H, dtype=q.dtype, device=q.device).index_add(0, col, w)
    out = torch.zeros_like(q[:num_nodes]).index_add(0, col, (w / lsum[col]).unsqueeze(-1) * kv_c[srow, 1])
    return lsum, out

