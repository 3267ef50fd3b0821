"""``K = torch.ops.torch_hrt``: the reference's custom-op namespace, served by
libhet_amd.so.

The reference loads ``libtorch_hrt.so`` and calls its kernels as
``torch.ops.torch_hrt.<name>(...)`` (hrt/python/kernels/__init__.py:4-16; op list:
``m.def`` lines of hrt/include/DGLHackKernel/OpExport/*.inc.h).  This module
defines ops with the same names, argument order and argument meaning in the same
namespace and implements them by calling the C ABI of include/het_amd.h on the
current torch stream.  Tensor arguments are only unwrapped to device pointers
here; all arithmetic happens in the HIP library.  CPU tensors are rejected for
the compute ops (there is no CPU path); the five layout converters run the native
device-side builders (csrc/layouts.hip) on GPU tensors and torch index ops on CPU tensors.
"""
from __future__ import annotations

import collections
import ctypes as C
from collections import OrderedDict
from typing import Dict, List, Optional

import torch

from . import _lib, graph as _graph, plan as _plan

Tensor = torch.Tensor
NAMESPACE = "torch_hrt"
# HET_TORCH_HRT_LIB=<path to libtorch_hrt.so>: take the reference-named ops from the COMPILED registration object
# (csrc/torch_export.cpp, `make -C het_amd/csrc torch_hrt`; loaded as the reference loads its own library,
# hrt/python/kernels/__init__.py:4-16) instead of defining them here.  The functions below then only serve this package's
# own callers (layers, backend); K.<op> goes through the compiled dispatcher entry.
import os as _os
COMPILED_LIB = _os.environ.get("HET_TORCH_HRT_LIB") or None
if COMPILED_LIB:
    torch.ops.load_library(COMPILED_LIB)
    _libdef = None
else:
    _libdef = torch.library.Library(NAMESPACE, "DEF")
_registered: List[str] = []
# The library's own device memory (groupings, their construction scratch) comes from torch's caching allocator: inside
# torch.cuda.memory_allocated, returned to torch's pool on eviction, no hipFree on an op's path (include/het_amd.h:
# het_set_allocator).  HET_TORCH_ALLOCATOR=0: hipMalloc, as a caller of the bare C ABI gets.
if _os.environ.get("HET_TORCH_ALLOCATOR", "1") != "0" and torch.cuda.is_available():
    _lib.use_torch_allocator()


def _p(t: Optional[Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(t: Tensor):
    """The current stream of the tensor's device as the raw hipStream_t (an int: the C entry points take it as void*).  The raw
    getter skips building a torch.cuda.Stream object per call -- host time per launch is what a rank's step at 8 ranks and a
    sampled block's step are made of (exp/host_profile_rank.py)."""
    if _raw_stream is not None:
        return _raw_stream(t.device.index)
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _chk(name: str, floats=(), ints=()):
    for t in floats:
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise _lib.HetError(f"{name}: expected contiguous float32 GPU tensors, got {t.dtype} on {t.device}"
                                f"{'' if t.is_contiguous() else ' (non-contiguous)'}")
    for t in ints:
        if not (t.is_cuda and t.dtype == torch.int64 and t.is_contiguous()):
            raise _lib.HetError(f"{name}: expected contiguous int64 GPU tensors, got {t.dtype} on {t.device}")


def _written_positions(schema: str):
    """Positions of the arguments a schema marks as written (``Tensor(a!) name``)."""
    params = schema[schema.index("(") + 1:schema.rindex(") ->")]
    out, depth, cur, pos = [], 0, "", 0
    for ch in params + ",":
        if ch == "," and depth == 0:
            if "!" in cur:
                out.append(pos)
            cur, pos = "", pos + 1
            continue
        depth += ch == "("
        depth -= ch == ")"
        cur += ch
    return tuple(out)


def _op(schema: str):
    name = schema.split("(")[0]
    written = _written_positions(schema)

    def deco(fn):
        impl = fn
        if written:
            # The dispatcher does not bump the version counter of a custom op's ``(a!)`` arguments, and the library writes through
            # raw pointers: caches keyed by (data_ptr, numel, _version) -- scale_in_rank_order, the sorted exp stream of a4 / a5 --
            # would keep serving a copy of a buffer that another op of this library has refilled in place.  Bumped
            # BEFORE the call, so that what the op itself records about its outputs (the sorted stream's key) is the new version.
            def impl(*args, **kwargs):
                for i in written:
                    t = args[i] if i < len(args) else None
                    if isinstance(t, Tensor):
                        try:
                            torch.autograd.graph.increment_version(t)
                        except RuntimeError:  # (an inference tensor: no version counter to keep)
                            pass
                return fn(*args, **kwargs)
        if _libdef is not None:
            _libdef.define(schema)
            _libdef.impl(name, impl, "CompositeExplicitAutograd")
        elif not hasattr(getattr(torch.ops, NAMESPACE), name):
            raise _lib.HetError(f"{COMPILED_LIB} does not register torch_hrt.{name}")
        _registered.append(name)
        return fn

    return deco


# Optional per-entry-point device timing (bench.py): name -> list of (start, end, args) with events recorded on
# the stream the kernels are launched on.  Empty = no overhead.
event_timers: Dict[str, list] = {}


def _call(dev_tensor: Tensor, cname: str, *args):
    if not event_timers and dev_tensor.device.index == torch.cuda.current_device():
        _lib.call(cname, *args)  # the common case: the tensor's device is current and nobody times the entry points
        return
    with torch.cuda.device(dev_tensor.device):
        rec = event_timers.get(cname)
        if rec is None:
            rec = event_timers.get("*")  # wildcard: time every entry point (bench.py's per-op breakdown)
            if rec is not None:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                _lib.call(cname, *args)
                b.record()
                rec.append((a, b, cname))
                return
        if rec is None:
            _lib.call(cname, *args)
            return
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.call(cname, *args)
        b.record()
        rec.append((a, b, args))


def _workspace(like: Tensor, query: str, *args, why: Optional[str] = None):
    """The scratch buffer of a C entry, sized by its byte-count query (include/het_amd.h: the het_*_workspace functions), asked on
    ``like``'s device: (float32 tensor there, or None for 0 bytes; the byte count to hand to the entry).  Every query answers in
    whole floats.  A negative answer raises, naming the query, with ``why`` or the library's message."""
    ask = getattr(_lib.lib(), query)
    if like.device.index == torch.cuda.current_device():
        nbytes = int(ask(*args))
    else:
        with torch.cuda.device(like.device):
            nbytes = int(ask(*args))
    if nbytes < 0:
        raise _lib.HetError(f"{query}: {why or _lib.lib().het_last_error().decode()}")
    return (torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=like.device) if nbytes else None), nbytes


# ------------------------------------------------------------------------------------
# info + layout converters
# ------------------------------------------------------------------------------------
@_op("build_debug_info() -> ()")
def build_debug_info():
    print(_lib.build_info())


@_op("transpose_csr(Tensor row_ptrs, Tensor col_indices, Tensor eids, Tensor rel_types) -> Tensor[]")
def transpose_csr(row_ptrs, col_indices, eids, rel_types):
    # DataConverters.inc.h:283-344: returns (row_ptrs, col_indices, eids, rel_types) of the transpose
    return list(_graph.transpose_csr(row_ptrs, col_indices, eids, rel_types))


@_op("convert_integrated_coo_to_separate_coo(Tensor row_indices, Tensor col_indices, Tensor rel_types, Tensor eids, "
     "int num_nodes, int num_rels) -> Tensor[]")
def convert_integrated_coo_to_separate_coo(row_indices, col_indices, rel_types, eids, num_nodes, num_rels):
    # DataConverters.inc.h:216-281 -> MyHyb.h:1047-1096 (bucket by relation; buckets kept in eid order)
    return list(_graph.integrated_coo_to_separate_coo(row_indices, col_indices, rel_types, eids, num_rels))


@_op("convert_integrated_csr_to_separate_coo(Tensor row_ptrs, Tensor col_indices, Tensor rel_types, Tensor eids) -> Tensor[]")
def convert_integrated_csr_to_separate_coo(row_ptrs, col_indices, rel_types, eids):
    # DataConverters.inc.h:10-77 -> MyHyb.h:1099-1150
    rows = _graph.csr_to_coo_rows(row_ptrs)
    num_rels = int(rel_types.max().item()) + 1 if rel_types.numel() else 1
    return list(_graph.integrated_coo_to_separate_coo(rows, col_indices, rel_types, eids, num_rels))


def _separate_csr(rows, cols, rels, eids, num_rows, num_rels):
    # a CSR over the composite row (relation, row): stable, so a row keeps its edges in input order
    row_ptrs, c, _, e = _graph.coo_to_csr(rels * num_rows + rows, cols, rels, eids, num_rows * num_rels)
    rel_ptrs = row_ptrs[::num_rows].contiguous()
    return [rel_ptrs, row_ptrs, c, e]


@_op("convert_integrated_csr_to_separate_csr(Tensor row_ptrs, Tensor col_indices, Tensor rel_types, Tensor eids) -> Tensor[]")
def convert_integrated_csr_to_separate_csr(row_ptrs, col_indices, rel_types, eids):
    # DataConverters.inc.h:79-145: one CSR per relation, row pointers concatenated ([R*N+1])
    rows = _graph.csr_to_coo_rows(row_ptrs)
    num_rels = int(rel_types.max().item()) + 1 if rel_types.numel() else 1
    return _separate_csr(rows, col_indices, rel_types, eids, row_ptrs.numel() - 1, num_rels)


@_op("convert_integrated_coo_to_separate_csr(Tensor row_indices, Tensor col_indices, Tensor rel_types, Tensor eids, "
     "int num_nodes, int num_rels) -> Tensor[]")
def convert_integrated_coo_to_separate_csr(row_indices, col_indices, rel_types, eids, num_nodes, num_rels):
    # DataConverters.inc.h:147-214
    return _separate_csr(row_indices, col_indices, rel_types, eids, num_nodes, num_rels)


# ------------------------------------------------------------------------------------
# segment GEMM ops
# ------------------------------------------------------------------------------------
def _matmul_lists(d: Dict[str, Tensor], kind: int):
    if kind == 0:
        return d["separate_coo_rel_ptrs"], d["separate_coo_node_indices"], d["separate_coo_eids"]
    if kind == 1:
        return d["unique_srcs_and_dests_rel_ptrs"], d["unique_srcs_and_dests_node_indices"], None
    raise _lib.HetError(f"rgnn_relational_matmul: CompactAsOfNodeKind {kind} not supported "
                        "(the reference asserts, RGNNOps.inc.h:292-294)")


@_op("rgnn_relational_matmul(Dict(str, Tensor) args_tensor_dict, int IntKind, Tensor weights, Tensor node_feat, "
     "Tensor(a!) ret, bool InputNumHeadOneFlag) -> ()")
def rgnn_relational_matmul(args_tensor_dict, IntKind, weights, node_feat, ret, InputNumHeadOneFlag):
    rp, g, s = _matmul_lists(args_tensor_dict, IntKind)
    _chk("rgnn_relational_matmul", (weights, node_feat, ret), tuple(t for t in (rp, g, s) if t is not None))
    R, H, K, D = weights.shape
    grp = ws = None
    X = H * D
    mfma = K in (32, 64, 128) and X in (32, 64, 128)
    # distinct (relation, node) rows + broadcast: the row-dot shape (D == 1), and projections the matrix-core kernel does
    # not take (e.g. an 8-wide output layer)
    if (IntKind == 0 and InputNumHeadOneFlag and ((D == 1 and H & (H - 1) == 0) or (D > 1 and not mfma and X & (X - 1) == 0 and X <= 256))
            and _plan.is_enabled() and ret.is_cuda and g.numel() > 0 and g.data_ptr() != s.data_ptr()):
        grp = _plan.get_grouping(rp, g, node_feat.shape[0], s, None)  # the grouping the backward uses as well
        if grp is not None:
            ws = torch.empty(max(1, grp.num_segments) * X, dtype=torch.float32, device=ret.device)
    _call(ret, "het_rgnn_relational_matmul", IntKind, _p(rp), R, _p(g), _p(s), g.numel(), _p(weights), _p(node_feat),
          _p(ret), H, K, D, int(InputNumHeadOneFlag), None if grp is None else grp.handle, _p(ws),
          0 if ws is None else ws.numel() * 4, _stream(ret))


def matmul_attn_dot_ok(H: int, K: int, D: int) -> bool:
    """Shapes het_rgnn_relational_matmul_attn_dot covers (the MFMA forward with the dot epilogue)."""
    return K in (32, 64, 128) and H * D in (32, 64, 128) and D >= 4 and D & (D - 1) == 0


def matmul_attn_dot_only_ok(args_tensor_dict, weights, node_feat) -> bool:
    """Whether the attention term can be formed without materialising the per-edge projection (kind 0 lists)."""
    R, H, K, D = weights.shape
    rp, g, s = _matmul_lists(args_tensor_dict, 0)
    return (_plan.is_enabled() and node_feat.is_cuda and matmul_attn_dot_ok(H, K, D) and H & (H - 1) == 0 and H <= H * D // 4
            and g.numel() > 0 and g.data_ptr() != s.data_ptr())


def matmul_attn_dot(args_tensor_dict, IntKind, weights, node_feat, ret, dot_w, dot_out, keep_rows=False, dot_rows=None):
    """rgnn_relational_matmul (one input head) that also writes dot_out[row, h] = <ret[row, h, :], dot_w[r, h, :]>.
    ret None: only dot_out (needs matmul_attn_dot_only_ok).  keep_rows: also return the [S, H, D] distinct projected
    rows of the (relation, node) grouping (None when that path is not taken).  dot_rows [E] int64: the dot of
    position i goes to dot_out[dot_rows[i]] instead of its separate_coo_eids row (grouping path only)."""
    rp, g, s = _matmul_lists(args_tensor_dict, IntKind)
    _chk("rgnn_relational_matmul_attn_dot", tuple(t for t in (weights, node_feat, ret, dot_w, dot_out) if t is not None),
         tuple(t for t in (rp, g, s) if t is not None))
    R, H, K, D = weights.shape
    grp = ws = comp = None
    if IntKind == 0 and _plan.is_enabled() and g.numel() > 0 and g.data_ptr() != s.data_ptr():
        grp = _plan.get_grouping(rp, g, node_feat.shape[0], s, None)  # the grouping the backward uses as well
        if grp is not None:
            S = max(1, grp.num_segments)
            if keep_rows or ret is None:
                comp = torch.empty((S, H, D), dtype=torch.float32, device=dot_out.device)
            ws = torch.empty(S * ((0 if comp is not None else H * D) + H), dtype=torch.float32, device=dot_out.device)
    if (ret is None or dot_rows is not None) and grp is None:
        raise _lib.HetError("rgnn_relational_matmul_attn_dot: ret=None / dot_rows need the (relation, node) grouping")
    dgrp = None if dot_rows is None else _plan.get_grouping(rp, g, node_feat.shape[0], dot_rows, None)
    _call(dot_out, "het_rgnn_relational_matmul_attn_dot", IntKind, _p(rp), R, _p(g), _p(s), g.numel(), _p(weights), _p(node_feat),
          _p(ret), _p(dot_w), _p(dot_out), H, K, D, None if grp is None else grp.handle, _p(ws),
          0 if ws is None else ws.numel() * 4, _p(comp), None if dgrp is None else dgrp.handle, _stream(dot_out))
    return comp


def matmul_attn_dot_rows(rel_ptrs, gather_idx, scatter_idx, weights, node_feat, ret, dot_w, dot_out):
    """ret[scatter_idx[i]] = node_feat[gather_idx[i]] . W[r(i)] and dot_out[scatter_idx[i], h] = <that row's head h, dot_w[r, h]> for
    a relation-bucketed list of DISTINCT rows -- no grouping is looked up or built (a piece of a unique (relation, node) list:
    the projection of the halo rows that have arrived, het_amd/backend/rgat_fused_layer.py)."""
    _chk("rgnn_relational_matmul_attn_dot", (weights, node_feat, ret, dot_w, dot_out), (rel_ptrs, gather_idx, scatter_idx))
    R, H, K, D = weights.shape
    if gather_idx.numel() == 0:
        return
    _call(dot_out, "het_rgnn_relational_matmul_attn_dot", 0, _p(rel_ptrs), R, _p(gather_idx), _p(scatter_idx), gather_idx.numel(),
          _p(weights), _p(node_feat), _p(ret), _p(dot_w), _p(dot_out), H, K, D, None, None, 0, None, None, _stream(dot_out))


def rows_add_bias(a, b=None, bias=None):
    """out = a (+ b) (+ bias broadcast over rows) in one pass (include/het_amd.h: het_rows_add_bias)."""
    _chk("rows_add_bias", tuple(t for t in (a, b, bias) if t is not None))
    out = torch.empty_like(a)
    _call(a, "het_rows_add_bias", _p(a), _p(b), _p(bias), _p(out), a.shape[0], a.numel() // max(1, a.shape[0]), _stream(a))
    return out


def rows_gather(x, idx):
    """out[i, :] = x[idx[i], :] (include/het_amd.h: het_rows_gather); torch.index_select off the GPU or for odd widths."""
    if not (x.is_cuda and x.dim() == 2 and x.shape[1] % 4 == 0 and x.dtype == torch.float32 and x.is_contiguous()):
        return x.index_select(0, idx)
    _chk("rows_gather", (x,), (idx,))
    out = torch.empty((idx.numel(), x.shape[1]), dtype=x.dtype, device=x.device)
    _call(x, "het_rows_gather", _p(x), _p(idx), idx.numel(), x.shape[1], _p(out), _stream(x))
    return out


def rows_scatter_add_(out, idx, src):
    """out[idx[i], :] += src[i, :] in place (het_rows_scatter_add); Tensor.index_add_ off the GPU."""
    if not (out.is_cuda and out.dim() == 2 and out.dtype == torch.float32 and out.is_contiguous() and src.is_contiguous()):
        return out.index_add_(0, idx, src)
    _chk("rows_scatter_add", (out, src), (idx,))
    X = out.shape[1]
    if _plan.is_enabled() and idx.numel() > 0 and 4 <= X <= 256 and X & (X - 1) == 0:
        # idx is a per-plan list (the halo send list): grouped by destination row once, then summed without atomics
        pos = _derived_get("positions", (idx,), lambda: torch.arange(idx.numel(), dtype=torch.int64, device=idx.device))
        g = _plan.get_grouping(None, idx, out.shape[0], pos, None)
        _call(out, "het_rows_scatter_add_grouped", g.handle, _p(src), X, _p(out), out.shape[0], _stream(out))
        return out
    _call(out, "het_rows_scatter_add", _p(src), _p(idx), idx.numel(), X, _p(out), _stream(out))
    return out


def matmul_attn_dot_only_backward(args_tensor_dict, weights_transposed, node_feat, dot_w, grad_dot, grad_node_feat, grad_weights,
                                  comp_rows=None, grad_dot_w=None, accumulate=False):
    """Backward of matmul_attn_dot when only dot_out was used (see include/het_amd.h); returns False when the fast
    path does not apply (no grouping / shape), leaving the outputs untouched."""
    rp, g, s = _matmul_lists(args_tensor_dict, 0)
    R, H, D, K = weights_transposed.shape
    if not (_plan.is_enabled() and H & (H - 1) == 0 and D % 4 == 0 and g.numel() > 0):
        return False
    grp = _plan.get_grouping(rp, g, node_feat.shape[0], s, None)
    if grp is None:
        return False
    _chk("backward_rgnn_relational_matmul_attn_dot_only", (weights_transposed, node_feat, dot_w, grad_dot, grad_node_feat, grad_weights), (rp, g, s))
    S = max(1, grp.num_segments)
    ws = torch.empty(((S * H + 3) // 4) * 4 + S * H * D, dtype=torch.float32, device=grad_dot.device)
    _call(grad_dot, "het_backward_rgnn_relational_matmul_attn_dot_only", _p(rp), R, _p(g), _p(s), g.numel(), node_feat.shape[0],
          _p(weights_transposed), _p(node_feat), _p(dot_w), _p(grad_dot), _p(grad_node_feat), _p(grad_weights), H, K, D,
          int(accumulate), grp.handle, _p(ws), ws.numel() * 4, _p(comp_rows), _p(grad_dot_w), _stream(grad_dot))
    return True


@_op("backward_rgnn_relational_matmul(Dict(str, Tensor) args_tensor_dict, int IntKind, Tensor weights_transposed, "
     "Tensor node_feat, Tensor gradout, Tensor(a!) grad_node_feat, Tensor(b!) grad_weights, bool InputNumHeadOneFlag) -> ()")
def backward_rgnn_relational_matmul(args_tensor_dict, IntKind, weights_transposed, node_feat, gradout, grad_node_feat,
                                    grad_weights, InputNumHeadOneFlag):
    matmul_backward(args_tensor_dict, IntKind, weights_transposed, node_feat, gradout, grad_node_feat, grad_weights,
                    InputNumHeadOneFlag, accumulate=True)


def matmul_backward(args_tensor_dict, IntKind, weights_transposed, node_feat, gradout, grad_node_feat, grad_weights,
                    InputNumHeadOneFlag, accumulate: bool, distinct_rows: bool = False):
    """backward_rgnn_relational_matmul with the choice of "+=" (the reference op's contract) or "=" outputs.
    distinct_rows (kind 1): the caller guarantees that the unique list holds a node at most once per relation -- the
    graph's own unique (relation, node) lists -- which lets the input gradients be added relation by relation with plain
    read-modify-write.  The reference-named op never sets it: any list, duplicates included, is then summed with float
    atomics as in the reference (include/het_amd.h, a2)."""
    rp, g, s = _matmul_lists(args_tensor_dict, IntKind)
    _chk("backward_rgnn_relational_matmul",
         tuple(t for t in (weights_transposed, node_feat, gradout, grad_node_feat, grad_weights) if t is not None),
         tuple(t for t in (rp, g, s) if t is not None))
    R, H, D, K = weights_transposed.shape
    grp, ws = None, None
    if IntKind == 0 and g.data_ptr() != s.data_ptr() and (InputNumHeadOneFlag or D > 1):
        grp = _plan.get_grouping(rp, g, node_feat.shape[0], s, None)
        if grp is not None:
            ws = torch.empty(max(1, grp.num_segments) * H * D, dtype=torch.float32, device=gradout.device)
    _call(gradout, "het_backward_rgnn_relational_matmul", IntKind, _p(rp), R, _p(g), _p(s), g.numel(),
          node_feat.shape[0], _p(weights_transposed), _p(node_feat), _p(gradout), _p(grad_node_feat), _p(grad_weights),
          H, K, D, int(InputNumHeadOneFlag), int(bool(accumulate)) | (2 if distinct_rows and IntKind == 1 else 0),
          None if grp is None else grp.handle, _p(ws),
          0 if ws is None else ws.numel() * 4, _stream(gradout))


@_op("rgnn_relational_matmul_no_scatter_gather_list(Tensor ntype_offset_ptrs, Tensor weights, Tensor inputs, "
     "Tensor(a!) ret) -> ()")
def rgnn_relational_matmul_no_scatter_gather_list(ntype_offset_ptrs, weights, inputs, ret):
    _chk("rgnn_relational_matmul_no_scatter_gather_list", (weights, inputs, ret), (ntype_offset_ptrs,))
    T, H, K, D = weights.shape
    n = inputs.shape[0]
    per_head = int(H > 1 and inputs.numel() == n * H * K)
    _call(ret, "het_rgnn_relational_matmul_no_scatter_gather_list", _p(ntype_offset_ptrs), T, n, _p(weights),
          _p(inputs), _p(ret), H, K, D, per_head, _stream(ret))


@_op("backward_rgnn_relational_matmul_no_scatter_gather_list(Tensor ntype_offset_ptrs, Tensor weights_transposed, "
     "Tensor inputs, Tensor gradout, Tensor(a!) grad_input, Tensor(b!) grad_weights) -> ()")
def backward_rgnn_relational_matmul_no_scatter_gather_list(ntype_offset_ptrs, weights_transposed, inputs, gradout,
                                                           grad_input, grad_weights):
    matmul_no_scatter_gather_backward(ntype_offset_ptrs, weights_transposed, inputs, gradout, grad_input, grad_weights,
                                      accumulate=True)


def matmul_no_scatter_gather_backward(ntype_offset_ptrs, weights_transposed, inputs, gradout, grad_input, grad_weights,
                                      accumulate: bool):
    _chk("backward_rgnn_relational_matmul_no_scatter_gather_list",
         tuple(t for t in (weights_transposed, inputs, gradout, grad_input, grad_weights) if t is not None), (ntype_offset_ptrs,))
    T, H, D, K = weights_transposed.shape
    n = inputs.shape[0]
    per_head = int(H > 1 and inputs.numel() == n * H * K)
    _call(gradout, "het_backward_rgnn_relational_matmul_no_scatter_gather_list", _p(ntype_offset_ptrs), T, n,
          _p(weights_transposed), _p(inputs), _p(gradout), _p(grad_input), _p(grad_weights), H, K, D, per_head,
          int(accumulate), _stream(gradout))


# ------------------------------------------------------------------------------------
# fused GAT (edge softmax + aggregation)
# ------------------------------------------------------------------------------------
def _gat_maps(kind: int, d: Dict[str, Tensor], backward: bool):
    """Flatten the op's dict into (row_a, row_b, col_a, col_b); key names as the launchers read them
    (RGATOps.inc.h:180-236 forward, :476-540 backward -- the backward spells the dual-list column
    pointer key 'unique_srcs_and_dests_rel_col')."""
    if kind == 0:
        return None, None, None, None
    if kind == 1:
        rp, nodes = d["unique_srcs_and_dests_rel_ptrs"], d["unique_srcs_and_dests_node_indices"]
        return rp, nodes, rp, nodes
    if kind == 3:
        rpc = d.get("unique_srcs_and_dests_rel_ptrs_col")
        if rpc is None:
            rpc = d["unique_srcs_and_dests_rel_col"]
        return (d["unique_srcs_and_dests_rel_ptrs"], d["unique_srcs_and_dests_node_indices_row"], rpc,
                d["unique_srcs_and_dests_node_indices_col"])
    if kind == 4:
        return d["edata_idx_to_inverse_idx_row"], None, d["edata_idx_to_inverse_idx_col"], None
    if kind == 2:  # one inverse index for both edge ends, as the reference's non-dual direct-indexing branch reads it
        m = d["edata_idx_to_inverse_idx"]
        return m, None, m, None
    raise _lib.HetError(f"relational_fused_gat: CompactAsOfNodeKind {kind} is not supported")


_derived: "OrderedDict[tuple, tuple]" = OrderedDict()
_DERIVED_MAX = 64
import threading as _threading
_derived_lock = _threading.RLock()


def _derived_get(tag, tensors, build):
    """Per-graph derived index tensors (row maps, relation of every position ...), built once and looked up by the
    identity of ALL the tensors they were derived from: (data_ptr, numel, _version) each, as het_amd/plan.py keys its
    groupings -- an in-place edit of any of them (a renumbering of the eids, a reordered block) misses the cache instead of
    returning stale rows.  The entry keeps the source tensors alive, which pins their storage (a data_ptr cannot be
    recycled for other contents while the entry lives).  Least recently used entries go first.
    A source that is an inference tensor has no version to miss on: such a lookup never hits and is never kept (plan.cacheable);
    and what ``build`` makes is a normal tensor in whatever mode the caller runs (plan.building): it is handed to later calls,
    training steps that save it for their backward among them."""
    key = (tag,) + tuple(_plan._ident(t) for t in tensors)
    with _derived_lock:  # (model threads and autograd workers share the cache: lookup, build and eviction under one lock)
        hit = _derived.get(key)
        if hit is None:
            with _plan.building():
                hit = (build(), tensors)
            if not _plan.cacheable(*key[1:]):
                return hit[0]
            _derived[key] = hit
            while len(_derived) > _DERIVED_MAX:
                _derived.popitem(last=False)
        else:
            _derived.move_to_end(key)
        return hit[0]


def _host_rel_ptrs(rel_ptrs: Tensor):
    """A relation-pointer list as a host int64 array, for the entries that read it on the host: one device read per list (cached by
    its identity), none per step."""
    lst = _derived_get("rel_ptrs_host", (rel_ptrs,), lambda: rel_ptrs.tolist())
    return (C.c_int64 * len(lst))(*lst)


def _rows_by_search(rel_ptrs, nodes, ua, ub):
    """Row of every (relation of the position, node) pair in the unique list (ua = its relation pointers, ub = node ids)."""
    R = rel_ptrs.numel() - 1
    bound = int(max(int(nodes.max().item()), int(ub.max().item()))) + 1
    rel_e = torch.repeat_interleave(torch.arange(R, device=nodes.device), rel_ptrs[1:] - rel_ptrs[:-1])
    rel_u = torch.repeat_interleave(torch.arange(R, device=nodes.device), ua[1:] - ua[:-1])
    return torch.searchsorted(rel_u * bound + ub, rel_e * bound + nodes).contiguous()


def _gat_direct(kind, maps, rel_ptrs, row, col, eids):
    """(kind, maps) as handed to the C entry points: the binary-search kinds 1 / 3 are turned into the direct-index
    kind 4 once per graph (feat / er row of every edge id, cached) -- the maps the kernels read without searching."""
    if kind == 2:
        return 4, maps  # (maps[2] is maps[0]: see _gat_maps)
    if kind not in (1, 3) or not _plan.is_enabled() or eids.numel() == 0:
        return kind, maps

    def build():
        srow = _src_rows_by_position(kind, maps, rel_ptrs, row, eids)
        drow = _dst_rows_by_position(kind, maps, rel_ptrs, col, eids)
        n = int(eids.max().item()) + 1
        mr = torch.empty(n, dtype=torch.int64, device=eids.device)
        mc = torch.empty(n, dtype=torch.int64, device=eids.device)
        mr[eids] = srow
        mc[eids] = drow
        return (mr, None, mc, None)

    return 4, _derived_get(("gatmap", kind), (maps[0], maps[1], maps[2], maps[3], rel_ptrs, row, col, eids), build)


def _src_rows_by_position(kind, maps, rel_ptrs, row, eids):
    """feat row of every edge position for the compact kinds (cached per graph)."""
    ra, rb = maps[0], maps[1]
    if kind == 4:
        return _derived_get("srow4", (ra, eids), lambda: ra[eids].contiguous())
    return _derived_get("srow", (ra, rb, rel_ptrs, row), lambda: _rows_by_search(rel_ptrs, row, ra, rb))


def _dst_rows_by_position(kind, maps, rel_ptrs, col, eids):
    """er row of every edge position for the compact kinds (cached per graph)."""
    ca, cb = maps[2], maps[3]
    if kind == 4:
        return _derived_get("drow4", (ca, eids), lambda: ca[eids].contiguous())
    return _derived_get("drow", (ca, cb, rel_ptrs, col), lambda: _rows_by_search(rel_ptrs, col, ca, cb))


def _csr_compact_maps(row_ptrs, col, eids, reltypes, uniq_rel_ptrs, uniq_nodes, rows_are_dst: bool):
    """CompactAsOfNodeFlag of the CSR GAT pair (RGATOps.inc.h:251-277, 430-460): feat / el / er live on the rows of ONE
    unique (relation, node) list and every edge end is looked up by (relation of the edge, node).  Turned once per graph
    (cached) into the direct-index maps of kind 4 -- feat row and er row of every EDGE ID -- which the destination-grouped
    kernels read without searching: (rows of the CSR expanded per position, {edata idx -> row} dict)."""
    def build():
        E = eids.numel()
        rows = _graph.csr_to_coo_rows(row_ptrs).contiguous()
        src, dst = (col, rows) if rows_are_dst else (rows, col)
        R = uniq_rel_ptrs.numel() - 1
        bound = int(max(int(row_ptrs.numel()) - 1, int(uniq_nodes.max().item()) + 1 if uniq_nodes.numel() else 1))
        rel_u = torch.repeat_interleave(torch.arange(R, device=col.device), uniq_rel_ptrs[1:] - uniq_rel_ptrs[:-1])
        keys = rel_u * bound + uniq_nodes
        n = int(eids.max().item()) + 1 if E else 0
        mr = torch.empty(n, dtype=torch.int64, device=col.device)
        mc = torch.empty(n, dtype=torch.int64, device=col.device)
        mr[eids] = torch.searchsorted(keys, reltypes * bound + src)
        mc[eids] = torch.searchsorted(keys, reltypes * bound + dst)
        return rows, {"edata_idx_to_inverse_idx_row": mr, "edata_idx_to_inverse_idx_col": mc}
    return _derived_get(("csrcompact", rows_are_dst), (row_ptrs, col, eids, reltypes, uniq_rel_ptrs, uniq_nodes), build)


def _csr_expanded_rows(row_ptrs, num_edges):
    """(row id of every CSR position, a one-relation rel_ptrs [0, E]) -- cached per CSR."""
    return _derived_get(("csr", num_edges), (row_ptrs,),
                        lambda: (_graph.csr_to_coo_rows(row_ptrs).contiguous(),
                                 torch.tensor([0, num_edges], dtype=torch.int64, device=row_ptrs.device)))


def _rel_by_position(rel_ptrs, num_positions):
    """Relation of every edge position of the separate COO (cached per graph)."""
    R = rel_ptrs.numel() - 1
    return _derived_get(("rel", num_positions), (rel_ptrs,),
                        lambda: torch.repeat_interleave(torch.arange(R, device=rel_ptrs.device), rel_ptrs[1:] - rel_ptrs[:-1],
                                                        output_size=num_positions).contiguous())


def _by_dst(kind, maps, rel_ptrs, row, col, eids, num_nodes):
    """Positions grouped by destination; payload0 = edge id, payload1 = feat row (compact kinds) or the relation
    of the position (kind 0; read by the fold_attn_l backward)."""
    if not _plan.is_enabled():
        return None
    p1 = _rel_by_position(rel_ptrs, eids.numel()) if kind == 0 else _src_rows_by_position(kind, maps, rel_ptrs, row, eids)
    return _plan.get_grouping(None, col, num_nodes, eids, p1)


@_op("relational_fused_gat_separate_coo(Tensor separate_coo_eids, Tensor separate_coo_rel_ptrs, "
     "Tensor separate_coo_row_indices, Tensor separate_coo_col_indices, int IntKind, "
     "Dict(str, Tensor) args_tensor_dict, Tensor feat_src, Tensor el, Tensor er, Tensor(a!) sum, Tensor(b!) exp, "
     "Tensor(c!) ret, float slope) -> ()")
def relational_fused_gat_separate_coo(separate_coo_eids, separate_coo_rel_ptrs, separate_coo_row_indices,
                                      separate_coo_col_indices, IntKind, args_tensor_dict, feat_src, el, er, sum, exp,
                                      ret, slope):
    # kind 0 on the destination-grouped kernels: the pass also leaves a copy of exp in the grouping's order (sequential 16-byte
    # stores: +338 MB written on ogbn-mag), remembered against the identity of (exp, el, er) -- the backward op streams it
    # when the same tensors come back (_sorted_stream_*)
    exs = None
    if (A5_SORTED_STREAM and IntKind == 0 and slope >= 0 and _plan.is_enabled() and separate_coo_eids.numel() > 0 and exp.dim() >= 2
            and gat_grouped_shape_ok(sum.shape[1], ret.numel() // max(1, ret.shape[0] * sum.shape[1]))):
        exs = torch.empty((separate_coo_eids.numel(), sum.shape[1]), dtype=exp.dtype, device=exp.device)
    wrote = fused_gat_forward(separate_coo_eids, separate_coo_rel_ptrs, separate_coo_row_indices, separate_coo_col_indices,
                              IntKind, args_tensor_dict, feat_src, el, er, sum, exp, ret, slope, exs)
    _sorted_stream_put(exp, el, er, separate_coo_eids, separate_coo_col_indices, float(slope), exs if wrote else None)


def gat_grouped_shape_ok(H: int, D: int) -> bool:
    """Shapes the destination-grouped GAT kernels cover (fused_gat_grouped.hip: grouped_shape_ok)."""
    X = H * D
    return D >= 4 and D & (D - 1) == 0 and X & (X - 1) == 0 and X // 4 <= 64


def fused_gat_forward(separate_coo_eids, separate_coo_rel_ptrs, separate_coo_row_indices, separate_coo_col_indices,
                      IntKind, args_tensor_dict, feat_src, el, er, sum, exp, ret, slope, exp_sorted, el_sorted=None,
                      er_sorted=None):
    """relational_fused_gat_separate_coo plus the optional ``exp_sorted`` output ([E,H], exp in
    destination-grouped order) that lets the backward stream instead of gather.  el_sorted / er_sorted (kind 0): the
    attention terms already in that order (gat_rank_of_position); el, er, exp may then be None."""
    name = "relational_fused_gat_separate_coo"
    maps = _gat_maps(IntKind, args_tensor_dict, False)
    _chk(name, tuple(t for t in (feat_src, el, er, sum, exp, ret, el_sorted, er_sorted) if t is not None),
         (separate_coo_eids, separate_coo_rel_ptrs, separate_coo_row_indices, separate_coo_col_indices)
         + tuple(m for m in maps if m is not None))
    IntKind, maps = _gat_direct(IntKind, maps, separate_coo_rel_ptrs, separate_coo_row_indices, separate_coo_col_indices,
                                separate_coo_eids)
    E, N, H = separate_coo_eids.numel(), ret.shape[0], sum.shape[1]
    D = feat_src.numel() // (feat_src.shape[0] * H) if feat_src.numel() else ret.numel() // max(1, N * H)
    g = _by_dst(IntKind, maps, separate_coo_rel_ptrs, separate_coo_row_indices, separate_coo_col_indices,
                separate_coo_eids, N)
    _call(ret, "het_relational_fused_gat_separate_coo", _p(separate_coo_eids), _p(separate_coo_rel_ptrs),
          _p(separate_coo_row_indices), _p(separate_coo_col_indices), separate_coo_rel_ptrs.numel() - 1, E, N, IntKind,
          _p(maps[0]), _p(maps[1]), _p(maps[2]), _p(maps[3]), _p(feat_src), _p(el), _p(er), _p(sum), _p(exp), _p(ret),
          None if g is None else _p(exp_sorted), H, D, float(slope), None if g is None else g.handle, _p(el_sorted),
          _p(er_sorted), _stream(ret))
    return g is not None and exp_sorted is not None



# ---- the op-level a5 streams the sorted copy of exp its a4 left --------------------------------------------------------
# Called on their own (the reference's model code: RelationalFusedGatSeparateCOO, rgat_layers_and_funcs.py:262-330), a5 gathers
# exp / el / er by edge id in destination order: a 128-byte line per 16-byte record (0.41 of the HBM roofline, 21 GB of traffic
# for 13.9 GB of tensors).  The layer-private path avoids that with a destination-sorted copy of exp written by the forward;
# here the same copy is kept BETWEEN the two reference-named calls, keyed by the identity of the tensors the backward would
# otherwise read: (data_ptr, _version) of exp, el, er + the edge lists.  A weak reference per tensor makes a recycled address a
# miss (a dead tensor's storage may be handed out again); an in-place edit bumps _version: also a miss.  A miss = the gathers.
import weakref as _weakref
A5_SORTED_STREAM = _os.environ.get("HET_A5_SORTED_STREAM", "1") != "0"
_sorted_streams: "OrderedDict[tuple, tuple]" = OrderedDict()
_SORTED_STREAMS_MAX = 2  # (a [E,H] float tensor each: 338 MB on ogbn-mag)
sorted_stream_hits = 0   # (tests / bench: how often the backward op found its stream)


def _sorted_stream_key(exp, el, er, eids, col, slope):
    """The key, or None where one of the tensors is an inference tensor (no version counter: an edit in place could not be seen;
    there is no backward under torch.inference_mode() to stream the copy to either)."""
    idents = tuple(_plan._ident(t) for t in (exp, el, er, eids, col))
    if not _plan.cacheable(*idents):
        return None
    return (idents[0][:2],) + idents[1:] + (slope, exp.device.index)


def _sorted_stream_put(exp, el, er, eids, col, slope, exs):
    key = _sorted_stream_key(exp, el, er, eids, col, slope)
    if key is None:
        return
    with _derived_lock:
        _sorted_streams.pop(key, None)
        if exs is not None:
            # exp's version is taken AFTER the op wrote it (the C side writes through the raw pointer: no bump of its own)
            _sorted_streams[key] = (exs, exp._version, tuple(_weakref.ref(t) for t in (exp, el, er)))
            while len(_sorted_streams) > _SORTED_STREAMS_MAX:
                _sorted_streams.popitem(last=False)


def _sorted_stream_get(exp, el, er, eids, col, slope):
    global sorted_stream_hits
    if not (A5_SORTED_STREAM and _plan.is_enabled()) or exp is None or el is None or er is None:
        return None
    with _derived_lock:
        hit = _sorted_streams.get(_sorted_stream_key(exp, el, er, eids, col, slope))
        if hit is None:
            return None
        exs, version, refs = hit
        if exp._version != version or any(r() is None for r in refs):
            return None
        sorted_stream_hits += 1
        return exs


@_op("backward_relational_fused_gat_separate_coo(Tensor separate_coo_eids, Tensor separate_coo_rel_ptrs, "
     "Tensor separate_coo_row_indices, Tensor separate_coo_col_indices, int IntKind, "
     "Dict(str, Tensor) args_tensor_dict, Tensor feat_src, Tensor el, Tensor er, Tensor sum, Tensor exp, Tensor ret, "
     "Tensor gradout, Tensor(a!) grad_feat_src, Tensor(b!) grad_el, Tensor(c!) grad_er, float slope) -> ()")
def backward_relational_fused_gat_separate_coo(separate_coo_eids, separate_coo_rel_ptrs, separate_coo_row_indices,
                                               separate_coo_col_indices, IntKind, args_tensor_dict, feat_src, el, er,
                                               sum, exp, ret, gradout, grad_feat_src, grad_el, grad_er, slope):
    exs = _sorted_stream_get(exp, el, er, separate_coo_eids, separate_coo_col_indices, float(slope)) if IntKind == 0 else None
    fused_gat_backward(separate_coo_eids, separate_coo_rel_ptrs, separate_coo_row_indices, separate_coo_col_indices,
                       IntKind, args_tensor_dict, feat_src, el, er, sum, exp, ret, gradout, grad_feat_src, grad_el,
                       grad_er, slope, exs)


def fused_gat_backward(separate_coo_eids, separate_coo_rel_ptrs, separate_coo_row_indices, separate_coo_col_indices,
                       IntKind, args_tensor_dict, feat_src, el, er, sum, exp, ret, gradout, grad_feat_src, grad_el,
                       grad_er, slope, exp_sorted, fold_attn_l=None, grad_fold_attn_l=None, fold_row_rel_ptrs=None,
                       grad_el_sorted=None):
    """fold_attn_l [R,H,D]: also add grad_el[e,h] * fold_attn_l[r,h,:] into grad_feat_src (see include/het_amd.h).
    grad_el_sorted [E,H] (kind 0): grad_el in destination-grouped order (gat_rank_of_position); grad_el / grad_er
    may then be None."""
    name = "backward_relational_fused_gat_separate_coo"
    maps = _gat_maps(IntKind, args_tensor_dict, True)
    _chk(name, tuple(t for t in (feat_src, el, er, sum, exp, ret, gradout, grad_feat_src, grad_el, grad_er, grad_el_sorted,
                                 exp_sorted) if t is not None),
         (separate_coo_eids, separate_coo_rel_ptrs, separate_coo_row_indices, separate_coo_col_indices)
         + tuple(m for m in maps if m is not None))
    IntKind, maps = _gat_direct(IntKind, maps, separate_coo_rel_ptrs, separate_coo_row_indices, separate_coo_col_indices,
                                separate_coo_eids)
    E, N, H = separate_coo_eids.numel(), ret.shape[0], sum.shape[1]
    D = ret.numel() // max(1, N * H)
    g = _by_dst(0, maps, separate_coo_rel_ptrs, separate_coo_row_indices, separate_coo_col_indices,
                separate_coo_eids, N) if IntKind == 0 else None
    gs = gd = ws = None
    if IntKind != 0 and _plan.is_enabled() and slope >= 0 and gat_grouped_shape_ok(H, D) and E > 0:
        srow = _src_rows_by_position(IntKind, maps, separate_coo_rel_ptrs, separate_coo_row_indices, separate_coo_eids)
        drow = _dst_rows_by_position(IntKind, maps, separate_coo_rel_ptrs, separate_coo_col_indices, separate_coo_eids)
        gs = _plan.get_grouping(None, srow, feat_src.shape[0], separate_coo_eids, separate_coo_col_indices)
        gd = _plan.get_grouping(None, drow, er.shape[0], separate_coo_eids, None)
        ws = torch.empty(N * 2 * H + E * H, dtype=torch.float32, device=ret.device)
    if IntKind == 0 and g is not None and grad_fold_attn_l is not None:
        ws = torch.empty(64 * grad_fold_attn_l.numel(), dtype=torch.float32, device=ret.device)  # replicas of the weight gradient
    _call(ret, "het_backward_relational_fused_gat_separate_coo", _p(separate_coo_eids), _p(separate_coo_rel_ptrs),
          _p(separate_coo_row_indices), _p(separate_coo_col_indices), separate_coo_rel_ptrs.numel() - 1, E, N, IntKind,
          _p(maps[0]), _p(maps[1]), _p(maps[2]), _p(maps[3]), _p(feat_src), _p(el), _p(er), _p(sum), _p(exp), _p(ret),
          None if g is None else _p(exp_sorted), _p(gradout), _p(grad_feat_src), _p(grad_el), _p(grad_er), H, D,
          float(slope), None if g is None else g.handle, None if gs is None else gs.handle,
          None if gd is None else gd.handle, feat_src.shape[0], E if er is None else er.shape[0], _p(ws), 0 if ws is None else ws.numel() * 4,
          None if fold_attn_l is None else _p(fold_attn_l), None if grad_fold_attn_l is None else _p(grad_fold_attn_l),
          None if fold_row_rel_ptrs is None else _p(fold_row_rel_ptrs), _p(grad_el_sorted), _stream(ret))


def grouping_rank_of_position(g):
    """[E] int64: sorted rank of every position of grouping ``g`` (cached on the grouping object, built at plan time)."""
    r = getattr(g, "rank_of_position", None)
    if r is None:
        keys = g._keep[1]
        with _plan.building():  # (kept with the grouping: a normal tensor whatever the caller's mode)
            r = torch.empty(keys.numel(), dtype=torch.int64, device=keys.device)
        _call(r, "het_grouping_rank_of_position", g.handle, _p(r), _stream(r))
        g.rank_of_position = r  # lives (and is evicted) with the grouping
    return r


def rgat_runs_shape_ok(H: int, D: int) -> bool:
    """Shapes of the run-sum form of the compact RGAT pair (include/het_amd.h: het_rgat_aggregate_compact_runs): rows of 32 / 64 /
    128 floats, heads of at least 16."""
    X = H * D
    return X in (32, 64, 128) and D >= 16 and D & (D - 1) == 0 and X % D == 0


def rgat_compact_groupings(col, srow, drow, num_nodes, num_src_rows, num_dst_rows, rel_ptrs=None, drow_nodes=None,
                           drow_rel_ptrs=None):
    """The groupings of the compact RGAT passes (include/het_amd.h: het_rgat_aggregate_compact): (by destination, by feat row,
    by er row, None).  ``srow`` / ``drow`` [E] int64: feat row and er row of every edge position.
    With ``rel_ptrs`` (relation pointers of the positions; they are relation-major): the run-sum form
    (het_rgat_aggregate_compact_runs) -- (by destination, by feat row, None, by (destination, relation)).  That form needs the er
    rows to BE the distinct (relation, destination) pairs: ``drow_nodes`` [S_col] / ``drow_rel_ptrs`` [R+1] (the list the rows
    index) are checked against the edges once per list."""
    by_dst = _plan.get_grouping(None, col, num_nodes, srow, drow)
    by_srow = _plan.get_grouping(None, srow, num_src_rows, col, drow)
    if by_dst is None or by_srow is None:
        return None
    if rel_ptrs is not None and num_nodes * (rel_ptrs.numel() - 1) >= 2 ** 31:
        rel_ptrs = None  # (destination * R + relation does not fit the groupings' int32 keys: the per-edge form)
    if rel_ptrs is not None:
        R = rel_ptrs.numel() - 1

        def build():
            rel = torch.repeat_interleave(torch.arange(R, dtype=torch.int64, device=col.device), rel_ptrs[1:] - rel_ptrs[:-1])
            if drow_nodes is not None:
                ok = bool((drow_nodes[drow] == col).all()) and drow.numel() == rel.numel()
                if ok and drow_rel_ptrs is not None:
                    ok = bool(((drow >= drow_rel_ptrs[rel]) & (drow < drow_rel_ptrs[rel + 1])).all())
                if not ok:
                    raise _lib.HetError("rgat_compact_groupings: the run-sum form needs every er row to be the (relation, "
                                        "destination) pair of its edges")
            return (col * R + rel).contiguous()
        key = _derived_get("dst_rel_key", (col, rel_ptrs, drow) + ((drow_nodes,) if drow_nodes is not None else ()), build)
        return by_dst, by_srow, None, _plan.get_grouping(None, key, num_nodes * R, None, None)
    by_drow = _plan.get_grouping(None, drow, num_dst_rows, grouping_rank_of_position(by_srow), None)
    return by_dst, by_srow, by_drow, None


def rgat_aggregate_compact(groupings, feat_c, el_c, er_c, sum, ret, slope, h_inout=None, num_rels=None, attn_l=None,
                           feat_rel_ptrs=None):
    """h_inout [rows, H*D] (optional): ret's rows are also added into it in place (include/het_amd.h).  ``sum`` receives the
    log-sum-exp of every (destination, head) -- these two entry points subtract a running maximum (no overflow for any el + er).
    Groupings in the run-sum form (rgat_compact_groupings with rel_ptrs; ``num_rels`` required): returns (q_rows, q_sum, q_ref)
    for rgat_backward_compact.  attn_l [R,H,D] + feat_rel_ptrs [R+1] (relation pointers of the feat rows), run-sum form: el_c is
    <feat_c, attn_l[relation of the row]> and the pass may form it from the rows it gathers (include/het_amd.h)."""
    _chk("rgat_aggregate_compact", tuple(t for t in (feat_c, el_c, er_c, sum, ret, h_inout) if t is not None))
    if groupings[3] is not None:
        return _rgat_aggregate_compact_runs("rgat_aggregate_compact_runs", groupings, feat_c, el_c, er_c, sum, ret, slope, h_inout,
                                            num_rels, attn_l, feat_rel_ptrs)
    N, H = sum.shape[0], sum.shape[1]
    D = ret.numel() // max(1, N * H)
    ws, nbytes = _workspace(ret, "het_rgat_aggregate_compact_workspace", groupings[0].handle, H, D)  # (hub destinations only)
    _call(ret, "het_rgat_aggregate_compact", groupings[0].handle, _p(feat_c), _p(el_c), _p(er_c), _p(sum), _p(ret), N, H, D,
          float(slope), _p(h_inout), 0 if h_inout is None else h_inout.shape[0], _p(ws), nbytes, _stream(ret))
    return None


def _rgat_aggregate_compact_runs(name, groupings, feat_c, el_c, er_c, sum, ret, slope, h_inout, num_rels, attn_l, feat_rel_ptrs):
    """The run-sum form of rgat_aggregate_compact / _bf16 behind their tensor checks: the C entry is het_<name>.  Returns the run
    sums (q_rows, q_sum, q_ref), fp32 whatever the row type."""
    N, H = sum.shape[0], sum.shape[1]
    D = ret.numel() // max(1, N * H)
    S_col = er_c.shape[0]
    q_rows = torch.empty((S_col, H, D), dtype=ret.dtype, device=ret.device)
    q_sum, q_ref = torch.empty_like(er_c), torch.empty_like(er_c)
    ws, nbytes = _workspace(ret, "het_rgat_aggregate_compact_runs_workspace", groupings[0].handle, groupings[3].handle, int(num_rels),
                            H, D, _stream(ret))
    host_ptrs = None
    if attn_l is not None and feat_rel_ptrs is not None:
        _chk(name, (attn_l,), (feat_rel_ptrs,))
        host_ptrs = _host_rel_ptrs(feat_rel_ptrs)
    _call(ret, "het_" + name, groupings[0].handle, groupings[3].handle, int(num_rels), _p(feat_c), _p(el_c),
          _p(er_c), _p(sum), _p(ret), N, H, D, float(slope), _p(h_inout), 0 if h_inout is None else h_inout.shape[0],
          _p(q_rows), _p(q_sum), _p(q_ref), S_col, _p(attn_l) if host_ptrs is not None else None, host_ptrs, _p(ws), nbytes,
          _stream(ret))
    return q_rows, q_sum, q_ref


def _rgat_aggregate_compact_forward(name, groupings, feat_c, el_c, er_c, h_inout, slope, num_rels, attn_l, feat_rel_ptrs):
    """rgat_aggregate_compact_forward / _bf16 behind their tensor checks: the C entry is het_<name>."""
    if groupings[3] is None:
        raise _lib.HetError(f"{name}: needs the groupings of the run-sum form (rgat_compact_groupings with rel_ptrs)")
    H, D = feat_c.shape[1], feat_c.shape[2]
    ws, nbytes = _workspace(h_inout, "het_rgat_aggregate_compact_forward_workspace", groupings[0].handle, groupings[3].handle,
                            int(num_rels), H, D, _stream(h_inout))
    host_ptrs = None
    if attn_l is not None and feat_rel_ptrs is not None:
        _chk(name, (attn_l,), (feat_rel_ptrs,))
        host_ptrs = _host_rel_ptrs(feat_rel_ptrs)
    _call(h_inout, "het_" + name, groupings[0].handle, groupings[3].handle, int(num_rels), _p(feat_c), _p(el_c), _p(er_c), H, D,
          float(slope), _p(h_inout), h_inout.shape[0], _p(attn_l) if host_ptrs is not None else None, host_ptrs, _p(ws), nbytes,
          _stream(h_inout))


def rgat_aggregate_compact_forward(groupings, feat_c, el_c, er_c, h_inout, slope, num_rels, attn_l=None, feat_rel_ptrs=None):
    """The forward of rgat_aggregate_compact's run-sum form when no backward follows (include/het_amd.h:
    het_rgat_aggregate_compact_forward): h_inout [rows, H*D] += the aggregated rows, in place, and nothing else is written -- no
    lse, no ret, no run sums.  ``groupings``: rgat_compact_groupings with rel_ptrs (the training forward's, shared with it)."""
    _chk("rgat_aggregate_compact_forward", (feat_c, el_c, er_c, h_inout))
    _rgat_aggregate_compact_forward("rgat_aggregate_compact_forward", groupings, feat_c, el_c, er_c, h_inout, slope, num_rels, attn_l,
                                    feat_rel_ptrs)


def rgat_attention_compact(groupings, el_c, er_c, slope, col, srow, drow, eids, num_nodes, lse_out=None, attn=None):
    """The attention weights of the compact RGAT layer (include/het_amd.h: het_rgat_attention_compact): attn [E,H] float32 with
    attn[eids[p], h] = softmax over the in-edges of col[p] of leaky(el_c[srow[p], h] + er_c[drow[p], h]) -- row p when ``eids`` is
    None.  ``groupings``: rgat_compact_groupings of the same (col, srow, drow); el_c [S_row,H] / er_c [S_col,H] float32 (the bf16
    layer's too).  ``lse_out`` [num_nodes,H] (optional) receives the log-sum-exp of every destination (-inf without in-edges).
    Returns attn (allocated unless given)."""
    ids = tuple(t for t in (col, srow, drow, eids) if t is not None)
    _chk("rgat_attention_compact", tuple(t for t in (el_c, er_c, lse_out, attn) if t is not None), ids)
    E, H = col.numel(), el_c.shape[1]
    if attn is None:
        attn = torch.empty((E, H), dtype=torch.float32, device=el_c.device)
    if (er_c.shape[1] != H or attn.shape != (E, H) or any(t.numel() != E for t in ids)
            or (lse_out is not None and lse_out.shape != (num_nodes, H))):
        raise _lib.HetError(f"rgat_attention_compact: el_c {tuple(el_c.shape)}, er_c {tuple(er_c.shape)}, attn {tuple(attn.shape)} and "
                            f"{E} edges / {num_nodes} nodes do not fit")
    if E == 0:
        return attn
    ws, nbytes = _workspace(attn, "het_rgat_attention_compact_workspace", groupings[0].handle, H, int(num_nodes), int(lse_out is not None),
                            why=f"rgat_attention_compact: unsupported shape H={H} (1, 2, 4 or 8 heads)")
    _call(attn, "het_rgat_attention_compact", groupings[0].handle, _p(el_c), _p(er_c), H, float(slope), _p(col), _p(srow), _p(drow),
          _p(eids), E, int(num_nodes), _p(lse_out), _p(attn), _p(ws), nbytes, _stream(attn))
    return attn


# ---- the RGAT layer's evaluation path with bf16 activations (backend/rgat_fused_layer.py: _forward_only_bf16) ----
def rgat_bf16_shape_ok(H: int, K: int, D: int) -> bool:
    """Shapes the bf16 evaluation path covers: the run-sum form's rows (32 / 64 / 128 wide, heads of at least 16), a (padded) input
    width of 32 / 64 / 128, and er from the folded weight through the one-head row-dot (1, 2, 4 or 8 heads)."""
    return rgat_runs_shape_ok(H, D) and K in (32, 64, 128) and H in (1, 2, 4, 8) and K >= 4 * H


def rgat_el_from_row(H: int, D: int, num_rels: int) -> bool:
    """Whether the run-sum walks form el from the feat row they gather (include/het_amd.h): el_c is then never read."""
    return D == 16 and num_rels <= 8


def rows_matmul_heads_bf16(rel_ptrs, gather_idx, weights, x, out):
    """out[i] = x[gather_idx[i]] . weights[r(i)] (het_rows_matmul_heads_bf16): x [*,K] and out [rows,H,D] bf16, weights [R,H,K,D] fp32."""
    _chk_bf16("rows_matmul_heads_bf16", (x, out), (weights,))
    _chk("rows_matmul_heads_bf16", (), (rel_ptrs, gather_idx))
    R, H, K, D = weights.shape
    n = gather_idx.numel()
    if x.shape[-1] != K or out.numel() != n * H * D or rel_ptrs.numel() != R + 1:
        raise _lib.HetError(f"rows_matmul_heads_bf16: x {tuple(x.shape)} / out {tuple(out.shape)} do not fit weights {tuple(weights.shape)} and {n} rows")
    _call(out, "het_rows_matmul_heads_bf16", _p(rel_ptrs), R, _p(gather_idx), n, _p(weights), _p(x), _p(out), H, K, D, _stream(out))


def rows_dot1h_bf16(rel_ptrs, gather_idx, weights, x, out):
    """out[i, h] = <x[gather_idx[i]], weights[r(i), h]> (het_rows_dot1h_bf16): x [*,K] bf16, weights [R,H,K] and out [rows,H] fp32."""
    _chk_bf16("rows_dot1h_bf16", (x,), (weights, out))
    _chk("rows_dot1h_bf16", (), (rel_ptrs, gather_idx))
    R, H, K = weights.shape
    n = gather_idx.numel()
    if x.shape[-1] != K or out.numel() != n * H or rel_ptrs.numel() != R + 1:
        raise _lib.HetError(f"rows_dot1h_bf16: x {tuple(x.shape)} / out {tuple(out.shape)} do not fit weights {tuple(weights.shape)} and {n} rows")
    _call(out, "het_rows_dot1h_bf16", _p(rel_ptrs), R, _p(gather_idx), None, n, _p(weights), _p(x), _p(out), H, K, _stream(out))


def rows_linear_bias_bf16(offsets, x, w, bias, out=None):
    """rows_linear_bias with bf16 rows (het_rows_linear_bias_bf16): x and out bf16, w [K,X] and bias [X] fp32; the bias is added in
    fp32 before the one rounding."""
    _chk_bf16("rows_linear_bias_bf16", tuple(t for t in (x, out) if t is not None), tuple(t for t in (w, bias) if t is not None))
    _chk("rows_linear_bias_bf16", (), (offsets,))
    shape = (x.shape[0], w.shape[1]) if out is None else tuple(out.shape)
    if x.shape[-1] != w.shape[0] or shape != (x.shape[0], w.shape[1]):
        raise _lib.HetError(f"rows_linear_bias_bf16: x {tuple(x.shape)} / out {shape} do not fit w {tuple(w.shape)}")
    return _rows_linear_bias("het_rows_linear_bias_bf16", offsets, x, w, bias, out)


def rgat_el_rows_bf16(rel_ptrs, feat_c, attn_l, el_c):
    """el_c[u,h] = <feat_c[u,h,:], attn_l[r(u),h,:]> from the rounded bf16 rows (het_rgat_el_rows_bf16): feat_c [S,H,D] bf16,
    attn_l [R,H,D] and el_c [S,H] fp32."""
    _chk_bf16("rgat_el_rows_bf16", (feat_c,), (attn_l, el_c))
    _chk("rgat_el_rows_bf16", (), (rel_ptrs,))
    S, H, D = feat_c.shape
    if attn_l.shape[1:] != (H, D) or el_c.shape != (S, H) or rel_ptrs.numel() != attn_l.shape[0] + 1:
        raise _lib.HetError("rgat_el_rows_bf16: shapes do not match")
    _call(el_c, "het_rgat_el_rows_bf16", _p(rel_ptrs), attn_l.shape[0], _p(feat_c), _p(attn_l), _p(el_c), S, H, D, _stream(el_c))


def rgat_aggregate_compact_forward_bf16(groupings, feat_c, el_c, er_c, h_inout, slope, num_rels, attn_l=None, feat_rel_ptrs=None):
    """rgat_aggregate_compact_forward over bf16 rows (het_rgat_aggregate_compact_forward_bf16): feat_c [S,H,D] and h_inout [rows, H*D]
    bf16, el_c / er_c / attn_l fp32.  ``el_c`` may be None where the walk forms el from the row it gathers (rgat_el_from_row)."""
    _chk_bf16("rgat_aggregate_compact_forward_bf16", (feat_c, h_inout), tuple(t for t in (el_c, er_c) if t is not None))
    _rgat_aggregate_compact_forward("rgat_aggregate_compact_forward_bf16", groupings, feat_c, el_c, er_c, h_inout, slope, num_rels,
                                    attn_l, feat_rel_ptrs)


# ---- the RGAT layer's training step with bf16 activations (backend/rgat_fused_layer.py: RgatLayerBf16Function) ----
def rgat_aggregate_compact_bf16(groupings, feat_c, el_c, er_c, sum, ret, slope, h_inout, num_rels, attn_l=None, feat_rel_ptrs=None):
    """rgat_aggregate_compact's run-sum form over bf16 rows (het_rgat_aggregate_compact_runs_bf16): feat_c [S,H,D] and h_inout
    [rows, H*D] bf16; el_c (the dots of the rounded rows: rgat_el_rows_bf16), er_c, sum [N,H], ret [N,H,D] and the returned run sums
    fp32.  h_inout receives the rows rgat_aggregate_compact_forward_bf16 would store."""
    name = "rgat_aggregate_compact_bf16"
    _chk_bf16(name, (feat_c, h_inout), (el_c, er_c, sum, ret))
    if groupings[3] is None:
        raise _lib.HetError(f"{name}: needs the groupings of the run-sum form (rgat_compact_groupings with rel_ptrs)")
    S, H, D = feat_c.shape
    N = sum.shape[0]
    if (el_c.shape != (S, H) or er_c.dim() != 2 or er_c.shape[1] != H or sum.shape != (N, H) or ret.shape != (N, H, D)
            or h_inout.dim() != 2 or h_inout.shape[1] != H * D or h_inout.shape[0] > N):
        raise _lib.HetError(f"{name}: feat_c {tuple(feat_c.shape)}, el_c {tuple(el_c.shape)}, er_c {tuple(er_c.shape)}, sum "
                            f"{tuple(sum.shape)}, ret {tuple(ret.shape)} and h_inout {tuple(h_inout.shape)} do not fit")
    return _rgat_aggregate_compact_runs("rgat_aggregate_compact_runs_bf16", groupings, feat_c, el_c, er_c, sum, ret, slope, h_inout,
                                        num_rels, attn_l, feat_rel_ptrs)


def rgat_backward_compact_bf16(groupings, feat_c, el_c, er_c, sum, ret, gradout, grad_feat_c, grad_el_c, grad_er_c, slope, runs,
                               drow_nodes, fold_attn_l=None, row_rel_ptrs=None, grad_bias=None, bias_rows=0, grad_attn_l=None,
                               finish_attn_grad=True):
    """rgat_backward_compact's run-sum form over bf16 rows (het_rgat_backward_compact_runs_bf16): feat_c [S,H,D] and gradout [N,H,D]
    bf16; everything else -- and every gradient -- fp32.  grad_bias [H*D]: the column sums of the first ``bias_rows`` gradout rows.
    ``finish_attn_grad``: as for rgat_backward_compact."""
    name = "rgat_backward_compact_bf16"
    _chk_bf16(name, (feat_c, gradout), tuple(t for t in (el_c, er_c, sum, ret, grad_feat_c, grad_el_c, grad_er_c, fold_attn_l, grad_bias,
                                                        grad_attn_l) + tuple(runs) if t is not None))
    _chk(name, (), tuple(t for t in (row_rel_ptrs, drow_nodes) if t is not None))
    S, H, D = feat_c.shape
    N = sum.shape[0]
    if (el_c.shape != (S, H) or er_c.dim() != 2 or er_c.shape[1] != H or sum.shape != (N, H) or ret.shape != (N, H, D)
            or gradout.shape != (N, H, D) or grad_feat_c.shape != (S, H, D) or grad_er_c.shape != er_c.shape
            or (grad_el_c is not None and grad_el_c.shape != (S, H)) or runs[0].shape != (er_c.shape[0], H, D)
            or (grad_bias is not None and (grad_bias.numel() != H * D or bias_rows > N))):
        raise _lib.HetError(f"{name}: feat_c {tuple(feat_c.shape)}, gradout {tuple(gradout.shape)}, sum {tuple(sum.shape)}, ret "
                            f"{tuple(ret.shape)}, er_c {tuple(er_c.shape)} and the gradients do not fit")
    return _rgat_backward_compact("het_rgat_backward_compact_runs%s_bf16", groupings, feat_c, el_c, er_c, sum, ret, gradout, grad_feat_c,
                                  grad_el_c, grad_er_c, slope, fold_attn_l, row_rel_ptrs, grad_bias, bias_rows, runs, drow_nodes, grad_attn_l,
                                  finish_attn_grad)


def rgat_node_backward_dx_bf16(n_begin, n_end, n_loop, grad_h, loop_wt, g_rows, weights_t, row_map, g_er, wa_t, dst_map, grad_x,
                               node_order=None):
    """rgat_node_backward_dx with bf16 activation rows (het_rgat_node_backward_dx_bf16): grad_h [n_loop, H*D] and grad_x [N,K] bf16,
    g_rows, g_er and the weights fp32; grad_x is rounded once, after every term of a node is summed."""
    name = "rgat_node_backward_dx_bf16"
    _chk_bf16(name, tuple(t for t in (grad_h, grad_x) if t is not None), tuple(t for t in (loop_wt, g_rows, weights_t, g_er, wa_t) if t is not None))
    R, H, D, K = weights_t.shape
    if (grad_x.dim() != 2 or grad_x.shape[1] != K or g_rows.shape[-1] != H * D or (grad_h is not None and (grad_h.shape[-1] != H * D
            or grad_h.shape[0] < min(int(n_loop), grad_x.shape[0]))) or row_map.shape != (R, grad_x.shape[0])):
        raise _lib.HetError(f"{name}: grad_x {tuple(grad_x.shape)}, g_rows {tuple(g_rows.shape)} and weights_t {tuple(weights_t.shape)} do not fit")
    _rgat_node_backward_dx("het_rgat_node_backward_dx_bf16", n_begin, n_end, n_loop, grad_h, loop_wt, g_rows, weights_t, row_map, g_er, wa_t,
                           dst_map, grad_x, node_order)


def rows_dot1h_backward_dw_bf16(rel_ptrs, gather_idx, x, gradout, grad_w, accumulate: bool):
    """grad_w[r(i), h] (+)= gradout[i, h] * x[gather_idx[i]] (het_rows_dot1h_backward_dw_bf16): the weight gradient of rows_dot1h_bf16;
    x [*,K] bf16, gradout [rows,H] and grad_w [R,H,K] fp32."""
    _chk_bf16("rows_dot1h_backward_dw_bf16", (x,), (gradout, grad_w))
    _chk("rows_dot1h_backward_dw_bf16", (), (rel_ptrs, gather_idx))
    R, H, K = grad_w.shape
    n = gather_idx.numel()
    if x.shape[-1] != K or gradout.numel() != n * H or rel_ptrs.numel() != R + 1:
        raise _lib.HetError(f"rows_dot1h_backward_dw_bf16: x {tuple(x.shape)} / gradout {tuple(gradout.shape)} do not fit grad_w "
                            f"{tuple(grad_w.shape)} and {n} rows")
    _call(grad_w, "het_rows_dot1h_backward_dw_bf16", _p(rel_ptrs), R, _p(gather_idx), None, n, _p(x), _p(gradout), _p(grad_w), H, K,
          int(accumulate), _stream(grad_w))


def rows_matmul_backward_split_ok(H: int, K: int, D: int) -> bool:
    """Shapes het_rows_matmul_backward_dx / _dw cover (one input head on the matrix cores)."""
    return K in (32, 64, 128) and H * D in (32, 64, 128)


def rows_matmul_backward_dx(rel_ptrs, gather_idx, weights_transposed, gradout, grad_x, atomic):
    """grad_x[gather_idx[i]] (+)= gradout[i] . Wt[r(i)] (include/het_amd.h: het_rows_matmul_backward_dx).  atomic: False "=",
    True "+=" with float atomics, 2 "+=" for lists whose rows are distinct inside every relation (unique (relation, node)
    lists): added relation by relation with plain read-modify-write."""
    _chk("rows_matmul_backward_dx", (weights_transposed, gradout, grad_x), (rel_ptrs,) + (() if gather_idx is None else (gather_idx,)))
    R, H, D, K = weights_transposed.shape
    _call(gradout, "het_rows_matmul_backward_dx", _p(rel_ptrs), R, _p(gather_idx), None, gradout.shape[0], _p(weights_transposed),
          _p(gradout), _p(grad_x), H, K, D, int(atomic), _stream(gradout))


def rows_matmul_backward_dw(rel_ptrs, gather_idx, x, gradout, grad_w, accumulate: bool, colsum: Optional[Tensor] = None):
    """grad_w[r(i)] (+)= x[gather_idx[i]]^T (x) gradout[i]; ``colsum`` [H*D] = SUM_i gradout[i] from the same pass
    (include/het_amd.h: het_rows_matmul_backward_dw, het_rows_matmul_backward_dw_colsum)."""
    _chk("rows_matmul_backward_dw", (x, gradout, grad_w) + (() if colsum is None else (colsum,)),
         (rel_ptrs,) + (() if gather_idx is None else (gather_idx,)))
    R, H, K, D = grad_w.shape
    if colsum is None:
        _call(gradout, "het_rows_matmul_backward_dw", _p(rel_ptrs), R, _p(gather_idx), None, gradout.shape[0], _p(x), _p(gradout),
              _p(grad_w), H, K, D, int(accumulate), _stream(gradout))
        return
    assert colsum.numel() == H * D, "rows_matmul_backward_dw: colsum must hold H*D floats"
    _call(gradout, "het_rows_matmul_backward_dw_colsum", _p(rel_ptrs), R, _p(gather_idx), None, gradout.shape[0], _p(x), _p(gradout),
          _p(grad_w), _p(colsum), H, K, D, int(accumulate), _stream(gradout))


def rgat_node_gemm_ok(R: int, H: int, K: int, D: int) -> bool:
    """Shapes of the node-major input-gradient pass (include/het_amd.h: het_rgat_node_backward_dx)."""
    return bool(_lib.lib().het_rgat_node_gemm_ok(R, H, K, D))


def node_row_map(rel_ptrs, nodes, num_nodes: int):
    """[R, num_nodes] int32: row of (relation, node) in a unique (relation, node) list, -1 where the node has none.  Built
    once per list on the device (het_node_row_map) and cached by the identity of the list."""
    def build():
        R = rel_ptrs.numel() - 1
        m = torch.empty((R, num_nodes), dtype=torch.int32, device=nodes.device)
        _call(nodes, "het_node_row_map", _p(rel_ptrs), R, _p(nodes), nodes.numel(), num_nodes, _p(m), _stream(nodes))
        return m
    _chk("node_row_map", (), (rel_ptrs, nodes))
    return _derived_get(("nodemap", num_nodes), (rel_ptrs, nodes), build)


def node_order_by_presence(row_map, dst_map=None, split=None):
    """[N] int32: the nodes sorted (stably) by which relations they have a row in -- tiles of 32 consecutive entries are then
    homogeneous and the node-major pass multiplies no zero rows (include/het_amd.h: node_order).  ``split``: nodes below it
    stay in front of the others (the owned / halo ranges of a partition are passed as two calls).  Cached per map."""
    def build():
        R, N = row_map.shape
        w = (1 << torch.arange(R, device=row_map.device, dtype=torch.int64)).view(R, 1)
        mask = ((row_map >= 0).to(torch.int64) * w).sum(0)
        if dst_map is not None:
            mask = mask | (((dst_map >= 0).to(torch.int64) * w).sum(0) << R)
        if split is not None:
            mask = mask | ((torch.arange(N, device=row_map.device) >= int(split)).to(torch.int64) << (2 * R))
        return torch.argsort(mask, stable=True).to(torch.int32).contiguous()
    return _derived_get(("node_order", None if split is None else int(split)), (row_map,) + (() if dst_map is None else (dst_map,)), build)


def rgat_node_backward_dx(n_begin, n_end, n_loop, grad_h, loop_wt, g_rows, weights_t, row_map, g_er, wa_t, dst_map, grad_x,
                          node_order=None):
    """grad_x rows [n_begin, n_end) of the one-node RGAT layer in one pass over the nodes (include/het_amd.h).  node_order
    (optional, [N] int32): the nodes of the call are the entries [n_begin, n_end) of this list."""
    _chk("rgat_node_backward_dx", tuple(t for t in (grad_h, loop_wt, g_rows, weights_t, g_er, wa_t, grad_x) if t is not None))
    _rgat_node_backward_dx("het_rgat_node_backward_dx", n_begin, n_end, n_loop, grad_h, loop_wt, g_rows, weights_t, row_map, g_er, wa_t,
                           dst_map, grad_x, node_order)


def _rgat_node_backward_dx(entry, n_begin, n_end, n_loop, grad_h, loop_wt, g_rows, weights_t, row_map, g_er, wa_t, dst_map, grad_x,
                           node_order):
    """rgat_node_backward_dx / _bf16 behind their tensor checks."""
    R, H, D, K = weights_t.shape
    _call(grad_x, entry, int(n_begin), int(n_end), int(n_loop), grad_x.shape[0], R, _p(grad_h), _p(loop_wt),
          _p(g_rows), _p(weights_t), _p(row_map), _p(g_er), _p(wa_t), _p(dst_map), _p(grad_x), H, K, D, _p(node_order),
          _stream(grad_x))


def node_rows_matmul_sum_ok(num_sources: int, KS: int, XO: int) -> bool:
    return bool(_lib.lib().het_node_rows_matmul_sum_ok(int(num_sources), int(KS), int(XO)))


def _node_rows_matmul_sum(entry, n_begin, n_end, sources, out, node_order, bias_slot):
    """The ctypes marshalling of het_node_rows_matmul_sum_bias / het_node_rows_matmul_sum_bf16 (``bias_slot``: the entry has one)."""
    N, XO = out.shape
    S = len(sources)
    KS = sources[0][3].shape[0]
    ptrs = (C.c_void_p * S)(*[src[0].data_ptr() + 4 * int(src[1]) for src in sources])
    strides = (C.c_int64 * S)(*[src[0].shape[1] if src[0].dim() == 2 else src[0].numel() // src[0].shape[0] for src in sources])
    maps = (C.c_void_p * S)(*[None if src[2] is None else src[2].data_ptr() for src in sources])
    ident = (C.c_int64 * S)(*[min(N, src[0].shape[0]) if src[2] is None else 0 for src in sources])
    wts = (C.c_void_p * S)(*[src[3].data_ptr() for src in sources])
    for src in sources:
        assert src[3].shape == (KS, XO) and src[3].is_contiguous() and (src[2] is None or (src[2].dtype == torch.int32 and src[2].numel() == N))
    _call(out, entry, int(n_begin), int(n_end), N, S, ptrs, strides, maps, ident, wts, *((None,) if bias_slot else ()), _p(out), KS, XO,
          _p(node_order), _stream(out))


def node_rows_matmul_sum(n_begin, n_end, sources, out, node_order=None):
    """out[n] = SUM_s rows_s[map_s[n]] . wt_s for the nodes at positions [n_begin, n_end) of node_order (include/het_amd.h:
    het_node_rows_matmul_sum).  sources: (rows [n_rows, W] float tensor, first column, map [N] int32 or None (row = node id),
    wt [KS, XO]) each; a source reads the KS columns of its rows that start at ``first column``."""
    _chk("node_rows_matmul_sum", tuple(t for src in sources for t in (src[0], src[3])) + (out,))
    _node_rows_matmul_sum("het_node_rows_matmul_sum_bias", n_begin, n_end, sources, out, node_order, True)


def rows_linear_bias_ok(K: int, X: int) -> bool:
    return K in (32, 64, 128) and X in (32, 64, 128)


def _rows_linear_bias(entry, offsets, x, w, bias, out):
    """rows_linear_bias / _bf16 behind their tensor checks: ``out`` (allocated unless given) has x's dtype."""
    if out is None:
        out = torch.empty((x.shape[0], w.shape[1]), dtype=x.dtype, device=x.device)
    _call(x, entry, _p(offsets), _p(x), _p(w), _p(bias), _p(out), x.shape[0], w.shape[0], w.shape[1], _stream(x))
    return out


def rows_linear_bias(offsets, x, w, bias, out=None):
    """x . w + bias for the rows [offsets[0], offsets[1]) of x (include/het_amd.h: het_rows_linear_bias).  ``out``: a tensor of the
    caller (e.g. allocated under another stream than the one the product is launched on)."""
    _chk("rows_linear_bias", tuple(t for t in (x, w, bias, out) if t is not None), (offsets,))
    return _rows_linear_bias("het_rows_linear_bias", offsets, x, w, bias, out)


# ---- typed LayerNorm over rows (HGT's use_norm; csrc/rows_layer_norm.hip): rows fp32 or bf16, everything else fp32 ----
def rows_layer_norm_ok(X: int) -> bool:
    """Row widths het_rows_layer_norm / _backward cover (a multiple of 4 in 4 .. 1024)."""
    return bool(_lib.lib().het_rows_layer_norm_ok(int(X)))


def _chk_f32_rows(name, rows, floats):
    _chk(name, tuple(rows) + tuple(floats))


def _ln_chk(name, chk_rows, offsets, rows, params, stats=()):
    """Tensor checks of the four layer-norm wrappers: ``rows`` [N,X] of the entry's row type, ``params`` [T,X] and ``stats`` [N] fp32."""
    chk_rows(name, rows, params + stats)
    _chk(name, (), (offsets,))
    N = rows[0].shape[0]
    if (params[0].dim() != 2 or any(t.shape != params[0].shape for t in params) or offsets.numel() != params[0].shape[0] + 1
            or any(t.shape != (N, params[0].shape[1]) for t in rows) or any(t.shape != (N,) for t in stats)):
        raise _lib.HetError(f"{name}: rows {[tuple(t.shape) for t in rows]}, statistics {[tuple(t.shape) for t in stats]} and offsets "
                            f"[{offsets.numel()}] do not fit the parameters {[tuple(t.shape) for t in params]}")


def _rows_layer_norm(entry, offsets, y, gamma, beta, eps, save_stats):
    N, T, X = y.shape[0], *gamma.shape
    out = torch.empty_like(y)
    mean = rstd = None
    if save_stats:
        mean = torch.empty(N, dtype=torch.float32, device=y.device)
        rstd = torch.empty(N, dtype=torch.float32, device=y.device)
    _call(y, entry, _p(offsets), T, _p(y), _p(gamma), _p(beta), float(eps), _p(out), _p(mean), _p(rstd), N, X, _stream(y))
    return out, mean, rstd


def _rows_layer_norm_backward(entry, offsets, y, gamma, mean, rstd, grad_out, want_y):
    N, T, X = y.shape[0], *gamma.shape
    grad_y = torch.empty_like(y) if want_y else None
    if N == 0:
        return grad_y, torch.zeros_like(gamma), torch.zeros_like(gamma)
    grad_gamma, grad_beta = torch.empty_like(gamma), torch.empty_like(gamma)
    ws, nbytes = _workspace(y, "het_rows_layer_norm_backward_workspace_bytes", N, T, X)
    _call(y, entry, _p(offsets), T, _p(y), _p(gamma), _p(mean), _p(rstd), _p(grad_out), _p(grad_y), _p(grad_gamma), _p(grad_beta),
          _p(ws), nbytes, N, X, _stream(y))
    return grad_y, grad_gamma, grad_beta


def rows_layer_norm(offsets, y, gamma, beta, eps=1e-5, save_stats=True):
    """(out [N,X], mean [N], rstd [N]) of het_rows_layer_norm: row v of run t of ``offsets`` [T+1] normalised over its X columns
    (biased variance) and scaled by gamma[t] / shifted by beta[t] ([T,X]).  ``save_stats=False``: mean and rstd are None and
    nothing is written for a backward."""
    _ln_chk("rows_layer_norm", _chk_f32_rows, offsets, (y,), (gamma, beta))
    return _rows_layer_norm("het_rows_layer_norm", offsets, y, gamma, beta, eps, save_stats)


def rows_layer_norm_backward(offsets, y, gamma, mean, rstd, grad_out, want_y=True):
    """(grad_y [N,X] or None, grad_gamma [T,X], grad_beta [T,X]) of het_rows_layer_norm_backward; the parameter gradients are summed
    without float atomics (the same bits every run)."""
    _ln_chk("rows_layer_norm_backward", _chk_f32_rows, offsets, (y, grad_out), (gamma,), (mean, rstd))
    return _rows_layer_norm_backward("het_rows_layer_norm_backward", offsets, y, gamma, mean, rstd, grad_out, want_y)


def rows_layer_norm_bf16(offsets, y, gamma, beta, eps=1e-5, save_stats=True):
    """rows_layer_norm with bf16 rows (het_rows_layer_norm_bf16): y and out bf16 (out rounded once at the store); gamma, beta, mean
    and rstd fp32."""
    _ln_chk("rows_layer_norm_bf16", _chk_bf16, offsets, (y,), (gamma, beta))
    return _rows_layer_norm("het_rows_layer_norm_bf16", offsets, y, gamma, beta, eps, save_stats)


def rows_layer_norm_backward_bf16(offsets, y, gamma, mean, rstd, grad_out, want_y=True):
    """rows_layer_norm_backward with bf16 rows (het_rows_layer_norm_backward_bf16): y, grad_out and grad_y bf16; gamma, mean, rstd
    and both parameter gradients fp32."""
    _ln_chk("rows_layer_norm_backward_bf16", _chk_bf16, offsets, (y, grad_out), (gamma,), (mean, rstd))
    return _rows_layer_norm_backward("het_rows_layer_norm_backward_bf16", offsets, y, gamma, mean, rstd, grad_out, want_y)


# ---- row-sparse embedding table (HET_RelGraphEmbed(sparse=True) + het_amd/optim.py RowSparseAdam; csrc/rows_embed.hip) ----
def rows_embed_ok(K: int) -> bool:
    """Row widths het_rows_embed_gather / _bf16 and het_rows_adam cover (a multiple of 4 in 4 .. 1024)."""
    return bool(_lib.lib().het_rows_embed_ok(int(K)))


def rows_embed_gather(table, rows, dtype=None, out=None):
    """out[i, :] = table[rows[i], :] of the fp32 table [N, K] as float32 (``dtype`` None / torch.float32) or, rounded once at the
    store, bfloat16 (het_rows_embed_gather / _bf16).  ``out``: a [B, K] tensor of the caller in that dtype with contiguous rows,
    16-byte (bf16: 8-byte) aligned -- refused before the launch otherwise."""
    dtype = torch.float32 if dtype is None else dtype
    if dtype not in (torch.float32, torch.bfloat16):
        raise _lib.HetError(f"rows_embed_gather: float32 or bfloat16 output rows, not {dtype}")
    _chk("rows_embed_gather", (table,), (rows,))
    if table.dim() != 2 or rows.dim() != 1:
        raise _lib.HetError(f"rows_embed_gather: a [N, K] table and a [B] id list, got {tuple(table.shape)} and {tuple(rows.shape)}")
    B, (N, K) = rows.numel(), table.shape
    if out is None:
        out = torch.empty((B, K), dtype=dtype, device=table.device)
    elif not (out.is_cuda and out.device == table.device and out.dtype == dtype and out.shape == (B, K) and out.is_contiguous()):
        raise _lib.HetError(f"rows_embed_gather: out must be a contiguous {dtype} [{B}, {K}] tensor on {table.device}")
    _call(table, "het_rows_embed_gather_bf16" if dtype == torch.bfloat16 else "het_rows_embed_gather", _p(table), _p(rows), B, N, K,
          _p(out), _stream(table))
    return out


def rows_adam_(p, exp_avg, exp_avg_sq, rows_sorted, perm, grad, lr, beta1, beta2, eps, step):
    """One lazy Adam step (torch.optim.SparseAdam's rule) in place on the rows of p, exp_avg, exp_avg_sq [N, K] that ``rows_sorted``
    [B] (ascending, repeats allowed) names; the gradient row of sorted position j is grad[perm[j]] (``perm`` None: grad[j]); ``step``:
    the 1-based count of this step (include/het_amd.h: het_rows_adam).  One launch, no atomics, no host synchronisation; the caller
    bumps p's version counter."""
    _chk("rows_adam", (p, exp_avg, exp_avg_sq, grad), tuple(t for t in (rows_sorted, perm) if t is not None))
    B = rows_sorted.numel()
    if (p.dim() != 2 or exp_avg.shape != p.shape or exp_avg_sq.shape != p.shape or grad.shape != (B, p.shape[1]) or rows_sorted.dim() != 1
            or (perm is not None and perm.shape != rows_sorted.shape)):
        raise _lib.HetError(f"rows_adam: p / exp_avg / exp_avg_sq [N, K], grad [B, K], rows_sorted / perm [B] expected, got "
                            f"{[tuple(t.shape) for t in (p, exp_avg, exp_avg_sq, grad, rows_sorted)]}")
    _call(p, "het_rows_adam", _p(p), _p(exp_avg), _p(exp_avg_sq), _p(rows_sorted), _p(perm), _p(grad), B, *p.shape, float(lr), float(beta1),
          float(beta2), float(eps), 1.0 - float(beta1) ** int(step), 1.0 - float(beta2) ** int(step), _stream(p))


# ---- keyed neighbour sampling and block construction (het_amd/sampling.py method="keyed"; csrc/block_sample.hip) ----
def sample_thresholds() -> Dict[str, int]:
    """The in-degrees at which het_sample_select changes its code path: ``workgroup_degree`` (a workgroup instead of a wave from
    here on) and ``chunk`` (positions per emission chunk of that workgroup)."""
    L = _lib.lib()
    return {"workgroup_degree": int(L.het_sample_workgroup_degree()), "chunk": int(L.het_sample_chunk())}


def sample_count(row_ptrs, dst, fanout: int):
    """(offsets [B + 1], total): the exclusive sum of min(deg, fanout) (deg when fanout <= 0) over the destinations ``dst`` of the
    in-CSR ``row_ptrs``, and its last entry on the host -- one read-back (het_sample_count)."""
    _chk("sample_count", (), (row_ptrs, dst))
    B = dst.numel()
    offsets = torch.empty(B + 1, dtype=torch.int64, device=dst.device)
    if B == 0:
        return offsets.zero_(), 0
    total = C.c_int64(0)
    _call(dst, "het_sample_count", _p(row_ptrs), _p(dst), B, row_ptrs.numel() - 1, int(fanout), _p(offsets), C.byref(total), _stream(dst))
    return offsets, int(total.value)


def sample_select(row_ptrs, dst, fanout: int, seed: int, draw: int, offsets, total: int):
    """(pos [total], owner [total]) of the edges the keyed rule keeps (het_sample_select); ``offsets`` / ``total`` from sample_count
    with the same arguments.  ``seed`` / ``draw``: any Python ints, taken modulo 2^64."""
    _chk("sample_select", (), (row_ptrs, dst, offsets))
    pos = torch.empty(total, dtype=torch.int64, device=dst.device)
    owner = torch.empty(total, dtype=torch.int64, device=dst.device)
    as_i64 = lambda v: ((int(v) & 0xFFFFFFFFFFFFFFFF) ^ (1 << 63)) - (1 << 63)  # noqa: E731  (the same 64 bits as a signed value)
    _call(dst, "het_sample_select", _p(row_ptrs), _p(dst), dst.numel(), row_ptrs.numel() - 1, int(fanout), as_i64(seed), as_i64(draw),
          _p(offsets), int(total), _p(pos), _p(owner), _stream(dst))
    return pos, owner


def block_renumber(src, pos, dst, node_map):
    """(nodes [B + num_extra], local_src [total]) of a block (het_block_renumber): ``dst`` (distinct ids) followed by the sampled
    sources ``src[pos]`` that are no destination, ascending; ``node_map`` [N] holds -1 everywhere before and after.  One read-back
    (the number of new nodes).  ``nodes`` is a view of a buffer of B + total ids."""
    _chk("block_renumber", (), (src, pos, dst, node_map))
    B, total = dst.numel(), pos.numel()
    if B == 0 or total == 0:
        return dst.clone(), torch.empty(0, dtype=torch.int64, device=dst.device)
    nodes = torch.empty(B + total, dtype=torch.int64, device=dst.device)
    local_src = torch.empty(total, dtype=torch.int64, device=dst.device)
    extra = C.c_int64(0)
    try:
        _call(dst, "het_block_renumber", _p(src), src.numel(), _p(pos), total, _p(dst), B, _p(node_map), node_map.numel(), _p(nodes),
              _p(local_src), C.byref(extra), _stream(dst))
    except _lib.HetError:
        node_map.fill_(-1)  # (a call that failed half way may have left marks behind)
        raise
    return nodes[: B + int(extra.value)], local_src


def block_relation_major(rel, eids, pos, owner, local_src, num_rels: int):
    """(rel_ptrs [R + 1], row, col, rel_types, edge_ids) of the kept edges in relation-major order, stable
    (het_block_relation_major): row = local source, col = owner, edge_ids = eids[pos]."""
    _chk("block_relation_major", (), (rel, eids, pos, owner, local_src))
    total, dev = pos.numel(), pos.device
    if total == 0:
        e = lambda: torch.empty(0, dtype=torch.int64, device=dev)  # noqa: E731
        return torch.zeros(int(num_rels) + 1, dtype=torch.int64, device=dev), e(), e(), e(), e()
    rel_ptrs = torch.empty(int(num_rels) + 1, dtype=torch.int64, device=dev)
    row, col, rel_out, eids_out = (torch.empty(total, dtype=torch.int64, device=dev) for _ in range(4))
    _call(pos, "het_block_relation_major", _p(rel), _p(eids), rel.numel(), _p(pos), _p(owner), _p(local_src), total, int(num_rels),
          _p(rel_ptrs), _p(row), _p(col), _p(rel_out), _p(eids_out), _stream(pos))
    return rel_ptrs, row, col, rel_out, eids_out


# ---- keyed dropout fused with the activation (het_amd/layers.py KeyedDropout; csrc/keyed_dropout.hip) ----
def keyed_dropout_params(p: float):
    """(T, scale) of the keyed dropout rule for a rate ``p`` in [0, 1): an element is dropped when its 16-bit field is below T, a kept
    one is multiplied by the float32 ``scale`` = 65536 / (65536 - T) (het_keyed_dropout_params; runs on the host)."""
    L = _lib.lib()
    T, scale = C.c_uint32(0), C.c_float(0.0)
    rc = L.het_keyed_dropout_params(float(p), C.byref(T), C.byref(scale))
    if rc != 0:
        raise _lib.HetError(f"het_keyed_dropout_params failed (code {rc}): {L.het_last_error().decode()}")
    return int(T.value), float(scale.value)


def _as_i64(v) -> int:
    return ((int(v) & 0xFFFFFFFFFFFFFFFF) ^ (1 << 63)) - (1 << 63)  # (the same 64 bits as a signed value)


def keyed_dropout_ok(*tensors) -> bool:
    """Whether the keyed dropout kernels take these tensors: contiguous float32 / bfloat16 on one GPU, 16-byte (bf16: 8-byte) aligned."""
    t0 = tensors[0]
    return all(t.is_cuda and t.device == t0.device and t.dtype == t0.dtype and t.dtype in (torch.float32, torch.bfloat16)
               and t.is_contiguous() and t.data_ptr() % (4 * t.element_size()) == 0 for t in tensors)


def _keyed_dropout_chk(name, tensors):
    if not keyed_dropout_ok(*tensors):
        raise _lib.HetError(f"{name}: expected contiguous float32 or bfloat16 GPU tensors of one dtype, 16-byte (bf16: 8-byte) aligned, got "
                            f"{[(t.dtype, str(t.device), t.is_contiguous(), t.data_ptr() % 16) for t in tensors]}")
    if any(t.shape != tensors[0].shape for t in tensors):
        raise _lib.HetError(f"{name}: tensors of one shape expected, got {[tuple(t.shape) for t in tensors]}")


def keyed_dropout(y, p, seed, draw, relu=False, base=0):
    """out = drop(a(y)) in one launch (het_keyed_dropout / _bf16): a = relu or the identity, the mask a pure function of
    (``seed``, ``draw``, ``base`` + the element's index in the contiguous tensor) -- the rule in include/het_amd.h.  ``seed`` / ``draw``:
    any Python ints, taken modulo 2^64; ``base``: a multiple of 4, at least 0."""
    _keyed_dropout_chk("keyed_dropout", (y,))
    out = torch.empty_like(y)
    _call(y, "het_keyed_dropout_bf16" if y.dtype == torch.bfloat16 else "het_keyed_dropout", _p(y), _p(out), y.numel(), int(base),
          int(bool(relu)), float(p), _as_i64(seed), _as_i64(draw), _stream(y))
    return out


def keyed_dropout_backward(grad_out, out, p, seed, draw, relu=False, base=0, grad_y=None):
    """The gradient of keyed_dropout's input (het_keyed_dropout_backward / _bf16) for the same (p, seed, draw, relu, base): ``out`` is
    the forward's result, read for relu only (None otherwise).  ``grad_y``: the tensor to write, which may be ``grad_out`` itself."""
    saved = (out,) if relu else ()
    if relu and out is None:
        raise _lib.HetError("keyed_dropout_backward: relu needs the forward's out")
    if grad_y is None:
        grad_y = torch.empty_like(grad_out)
    _keyed_dropout_chk("keyed_dropout_backward", (grad_out, grad_y) + saved)
    _call(grad_out, "het_keyed_dropout_backward_bf16" if grad_out.dtype == torch.bfloat16 else "het_keyed_dropout_backward", _p(grad_out),
          _p(out) if relu else None, _p(grad_y), grad_out.numel(), int(base), int(bool(relu)), float(p), _as_i64(seed), _as_i64(draw),
          _stream(grad_out))
    return grad_y


# ---- softmax cross-entropy over rows of logits (het_amd/layers.py SoftmaxCrossEntropy; csrc/softmax_xent.hip) ----
XENT_REDUCTIONS = {"mean": 0, "sum": 1}  # HET_XENT_MEAN / HET_XENT_SUM of include/het_amd.h


def softmax_xent_params() -> Dict[str, int]:
    """The launch constants of csrc/softmax_xent.hip (het_softmax_xent_params; runs on the host): ``lane_elems`` columns per lane
    before a row gets another lane, at most ``max_lanes`` lanes per row, at most ``max_blocks`` workgroups of ``block`` threads."""
    L = _lib.lib()
    out = (C.c_int64 * 4)()
    rc = L.het_softmax_xent_params(out)
    if rc != 0:
        raise _lib.HetError(f"het_softmax_xent_params failed (code {rc}): {L.het_last_error().decode()}")
    return dict(zip(("lane_elems", "max_lanes", "max_blocks", "block"), (int(v) for v in out)))


def softmax_xent_lanes(C_: int) -> int:
    """Lanes a row of ``C_`` logits gets: the power of two G with C_ <= G * lane_elems, at most max_lanes."""
    p = softmax_xent_params()
    g = 1
    while g < p["max_lanes"] and g * p["lane_elems"] < C_:
        g *= 2
    return g


def softmax_xent_thresholds():
    """The class counts up to which a row gets 1, 2, 4 ... lanes (one more column gives it twice as many)."""
    p = softmax_xent_params()
    out, g = [], 1
    while g < p["max_lanes"]:
        out.append(g * p["lane_elems"])
        g *= 2
    return tuple(out)


def softmax_xent_rows_per_pass(C_: int) -> int:
    """Rows a full grid takes before a wave takes a second one."""
    p = softmax_xent_params()
    return p["max_blocks"] * p["block"] // softmax_xent_lanes(C_)


def softmax_xent_ok(logits, labels=None) -> bool:
    """Whether the softmax cross-entropy kernels take these tensors: [N, C] contiguous float32 / bfloat16 logits on a GPU with C >= 1,
    16-byte (bf16: 8-byte) aligned, and [N] contiguous int64 labels on the same device."""
    return (logits.is_cuda and logits.dim() == 2 and logits.shape[1] >= 1 and logits.dtype in (torch.float32, torch.bfloat16)
            and logits.is_contiguous() and logits.data_ptr() % (4 * logits.element_size()) == 0
            and (labels is None or (labels.device == logits.device and labels.dtype == torch.int64 and labels.dim() == 1
                                    and labels.shape[0] == logits.shape[0] and labels.is_contiguous() and labels.data_ptr() % 8 == 0)))


def _softmax_xent_chk(name, logits, labels, reduction):
    if not softmax_xent_ok(logits, labels):
        raise _lib.HetError(f"{name}: expected contiguous float32 or bfloat16 GPU logits [N, C], 16-byte (bf16: 8-byte) aligned, and int64 "
                            f"labels [N] on the same device, got {logits.dtype} {tuple(logits.shape)} on {logits.device}"
                            f"{'' if logits.is_contiguous() else ' (non-contiguous)'} at offset {logits.data_ptr() % 16} and "
                            f"{labels.dtype} {tuple(labels.shape)} on {labels.device}")
    if reduction not in XENT_REDUCTIONS:
        raise _lib.HetError(f"{name}: reduction 'mean' or 'sum', not {reduction!r}")


def softmax_xent(logits, labels, ignore_index=-100, reduction="mean", want_lse=True):
    """(loss, lse, stats) of het_softmax_xent / _bf16: the fp32 scalar loss of the rule in include/het_amd.h, lse [N] fp32 for the
    backward (None with ``want_lse=False``) and stats int64 [3] = (valid, correct, bad rows), all on the device; nothing is read back."""
    _softmax_xent_chk("softmax_xent", logits, labels, reduction)
    return _softmax_xent(logits, labels, ignore_index, reduction, want_lse)


def _softmax_xent(logits, labels, ignore_index, reduction, want_lse):
    """softmax_xent behind its tensor checks (the autograd node has asked softmax_xent_ok once)."""
    N, C_ = logits.shape
    dev = logits.device
    lse = torch.empty(N, dtype=torch.float32, device=dev) if want_lse else None
    if N == 0:  # (no launch: the entry writes nothing)
        return (torch.full((), float("nan") if reduction == "mean" else 0.0, dtype=torch.float32, device=dev), lse,
                torch.zeros(3, dtype=torch.int64, device=dev))
    loss = torch.empty((), dtype=torch.float32, device=dev)
    stats = torch.empty(3, dtype=torch.int64, device=dev)
    ws, nbytes = _workspace(logits, "het_softmax_xent_workspace", N, C_)
    _call(logits, "het_softmax_xent_bf16" if logits.dtype == torch.bfloat16 else "het_softmax_xent", _p(logits), _p(labels), N, C_,
          int(ignore_index), XENT_REDUCTIONS[reduction], _p(loss), _p(lse), _p(stats), _p(ws), nbytes, _stream(logits))
    return loss, lse, stats


def softmax_xent_backward(logits, labels, lse, stats, grad_loss, ignore_index=-100, reduction="mean"):
    """grad_logits [N, C] in the logits' dtype (het_softmax_xent_backward / _bf16) for the forward's ``lse`` and ``stats``;
    ``grad_loss``: the fp32 scalar gradient of the loss, on the device (it is read there, like stats[0])."""
    _softmax_xent_chk("softmax_xent_backward", logits, labels, reduction)
    N, C_ = logits.shape
    _chk("softmax_xent_backward", (lse, grad_loss), (stats,))
    if lse.shape != (N,) or stats.shape != (3,) or grad_loss.numel() != 1 or any(t.device != logits.device for t in (lse, stats, grad_loss)):
        raise _lib.HetError(f"softmax_xent_backward: lse [{N}], stats [3] and a scalar grad_loss on {logits.device} expected, got "
                            f"{tuple(lse.shape)}, {tuple(stats.shape)}, {tuple(grad_loss.shape)}")
    return _softmax_xent_backward(logits, labels, lse, stats, grad_loss, ignore_index, reduction)


def _softmax_xent_backward(logits, labels, lse, stats, grad_loss, ignore_index, reduction):
    """softmax_xent_backward behind its tensor checks (the autograd node passes what its own forward made)."""
    N, C_ = logits.shape
    grad = torch.empty_like(logits)
    _call(logits, "het_softmax_xent_backward_bf16" if logits.dtype == torch.bfloat16 else "het_softmax_xent_backward", _p(logits),
          _p(labels), _p(lse), _p(stats), _p(grad_loss), N, C_, int(ignore_index), XENT_REDUCTIONS[reduction], _p(grad), _stream(logits))
    return grad


# ---- link prediction on triples: keyed corruption, the plan of a batch, the DistMult score (het_amd/linkpred.py; csrc/triple_score.hip) ----
_TRIPLE_PARAMS = ("min_width", "max_width", "max_lanes", "list_chunk", "rel_chunk", "max_blocks", "block")
TriplePlan = collections.namedtuple("TriplePlan", "node_ptr node_slots rel_ptr rel_order chunk_ptr bad num_nodes num_rels")


def triple_params() -> Dict[str, int]:
    """The launch constants of csrc/triple_score.hip (het_triple_params; runs on the host): the widths D served natively are the
    multiples of 4 from ``min_width`` to ``max_width``; a triple gets the power-of-two number of lanes G with D <= 4 G, at most
    ``max_lanes``; a node's slot list longer than ``list_chunk`` (L) is summed in chunks of L; grad_w in chunks of ``rel_chunk``."""
    L = _lib.lib()
    out = (C.c_int64 * len(_TRIPLE_PARAMS))()
    rc = L.het_triple_params(out)
    if rc != 0:
        raise _lib.HetError(f"het_triple_params failed (code {rc}): {L.het_last_error().decode()}")
    return dict(zip(_TRIPLE_PARAMS, (int(v) for v in out)))


def triple_lanes(D: int) -> int:
    """Lanes a triple (a node, a chunk) of width ``D`` gets."""
    p = triple_params()
    g = 1
    while g < p["max_lanes"] and 4 * g < D:
        g *= 2
    return g


def triple_lane_thresholds():
    """The widths up to which a triple gets 1, 2, 4 ... lanes (4 more columns give it twice as many)."""
    p = triple_params()
    out, g = [], 1
    while g < p["max_lanes"]:
        out.append(4 * g)
        g *= 2
    return tuple(out)


def triple_long_list() -> int:
    """L: a node with more slots than this has its gradient row summed in chunks of L."""
    return triple_params()["list_chunk"]


def triple_width_ok(D: int) -> bool:
    p = triple_params()
    return p["min_width"] <= D <= p["max_width"] and D % 4 == 0


def distmult_ok(h, w) -> bool:
    """Whether the DistMult kernels take these tables: h [N, D] contiguous float32 / bfloat16 on a GPU, 16-byte (bf16: 8-byte) aligned,
    w [R, D] contiguous float32 on the same device, D a width of triple_params(), N and R below 2^31 - 1."""
    return (h.is_cuda and h.dim() == 2 and w.dim() == 2 and h.dtype in (torch.float32, torch.bfloat16) and w.dtype == torch.float32
            and w.device == h.device and h.shape[1] == w.shape[1] and h.is_contiguous() and w.is_contiguous()
            and h.data_ptr() % (4 * h.element_size()) == 0 and w.data_ptr() % 16 == 0 and triple_width_ok(h.shape[1])
            and h.shape[0] < 2 ** 31 - 1 and w.shape[0] < 2 ** 31 - 1)


def _triple_ids_chk(name, like, *ids):
    n = ids[0].shape[0] if ids[0].dim() == 1 else -1
    for t in ids:
        if not (t.is_cuda and t.dtype == torch.int64 and t.dim() == 1 and t.shape[0] == n and t.is_contiguous() and t.data_ptr() % 8 == 0
                and (like is None or t.device == like.device)):
            raise _lib.HetError(f"{name}: expected contiguous int64 GPU id tensors of one length on one device, got {t.dtype} {tuple(t.shape)} "
                                f"on {t.device}")
    if n >= 2 ** 30:
        raise _lib.HetError(f"{name}: {n} triples (fewer than 2^30 expected)")


def _distmult_chk(name, h, w, s, r, o):
    if not distmult_ok(h, w):
        raise _lib.HetError(f"{name}: expected contiguous float32 or bfloat16 GPU rows h [N, D], 16-byte (bf16: 8-byte) aligned, and float32 "
                            f"w [R, D] on the same device with D a multiple of 4 in the widths of triple_params(), got {h.dtype} "
                            f"{tuple(h.shape)} on {h.device}{'' if h.is_contiguous() else ' (non-contiguous)'} and {w.dtype} {tuple(w.shape)} "
                            f"on {w.device}")
    _triple_ids_chk(name, h, s, r, o)


def _key_i64(v: int) -> int:
    """The 64 bits of a seed or draw number as the signed value the C entries take."""
    v = int(v) & ((1 << 64) - 1)
    return v - (1 << 64) if v >> 63 else v


def triple_corrupt(src, rel, dst, num_neg: int, seed: int, draw: int, node_type_offsets=None, num_nodes: int = 0):
    """(s, r, o), each [P * (1 + num_neg)] int64: the positives followed by their keyed corruptions (het_triple_corrupt; the rule in
    het_amd/linkpred.py).  One launch; ``node_type_offsets``: an int64 tensor on the positives' device, or None."""
    _triple_ids_chk("triple_corrupt", None, src, rel, dst)
    num_neg, num_nodes = int(num_neg), int(num_nodes)
    if num_neg < 0 or not 0 <= num_nodes < 2 ** 31:
        raise _lib.HetError(f"triple_corrupt: num_neg={num_neg} (at least 0), num_nodes={num_nodes} (below 2^31)")
    offs, ntypes = None, 0
    if node_type_offsets is not None:
        offs = node_type_offsets
        if not (offs.is_cuda and offs.device == src.device and offs.dtype == torch.int64 and offs.dim() == 1 and offs.numel() >= 2
                and offs.is_contiguous()):
            raise _lib.HetError(f"triple_corrupt: node_type_offsets is a contiguous int64 tensor [num_types + 1] on {src.device}, got "
                                f"{offs.dtype} {tuple(offs.shape)} on {offs.device}")
        ntypes = offs.numel() - 1
    P = src.shape[0]
    T = P * (1 + num_neg)
    if T >= 2 ** 30:
        raise _lib.HetError(f"triple_corrupt: {T} triples (fewer than 2^30 expected)")
    s, r, o = (torch.empty(T, dtype=torch.int64, device=src.device) for _ in range(3))
    if P:
        _call(src, "het_triple_corrupt", _p(src), _p(rel), _p(dst), P, num_neg, _key_i64(seed), _key_i64(draw), _p(offs), ntypes, num_nodes,
              _p(s), _p(r), _p(o), _stream(src))
    return s, r, o


def triple_plan(s, r, o, num_nodes: int, num_rels: int) -> TriplePlan:
    """The inverted index of a batch of triples (het_triple_plan): per node the ascending slots 2 j + side it owns, per relation its
    triples in ascending j, the chunk offsets of both and the device count of bad triples.  Nothing is read back."""
    _triple_ids_chk("triple_plan", None, s, r, o)
    return _triple_plan(s, r, o, int(num_nodes), int(num_rels))


def _triple_plan(s, r, o, N, R):
    T, dev = s.shape[0], s.device
    if not (0 <= N < 2 ** 31 - 1 and 0 <= R < 2 ** 31 - 1):
        raise _lib.HetError(f"triple_plan: num_nodes={N}, num_rels={R} (both below 2^31 - 1)")
    i64 = dict(dtype=torch.int64, device=dev)
    if T == 0:  # (no launch: the backward reads no plan)
        return TriplePlan(torch.zeros(N + 1, **i64), torch.zeros(0, **i64), torch.zeros(R + 1, **i64), torch.zeros(0, **i64),
                          torch.zeros(N + R + 2, **i64), torch.zeros(1, **i64), N, R)
    plan = TriplePlan(torch.empty(N + 1, **i64), torch.empty(2 * T, **i64), torch.empty(R + 1, **i64), torch.empty(T, **i64),
                      torch.empty(N + R + 2, **i64), torch.empty(1, **i64), N, R)
    ws, nbytes = _workspace(s, "het_triple_plan_workspace", T, N, R)
    _call(s, "het_triple_plan", _p(s), _p(r), _p(o), T, N, R, _p(plan.node_ptr), _p(plan.node_slots), _p(plan.rel_ptr), _p(plan.rel_order),
          _p(plan.chunk_ptr), _p(plan.bad), _p(ws), nbytes, _stream(s))
    return plan


def distmult_score(h, w, s, r, o):
    """score [T] fp32 = sum_d h[s, d] * w[r, d] * h[o, d] (het_distmult_score / _bf16; one launch); +0 for a triple with an id outside
    its table."""
    _distmult_chk("distmult_score", h, w, s, r, o)
    return _distmult_score(h, w, s, r, o)


def _distmult_score(h, w, s, r, o):
    T = s.shape[0]
    score = torch.empty(T, dtype=torch.float32, device=h.device)
    if T:
        _call(h, "het_distmult_score_bf16" if h.dtype == torch.bfloat16 else "het_distmult_score", _p(h), _p(w), _p(s), _p(r), _p(o), T,
              h.shape[0], w.shape[0], h.shape[1], _p(score), _stream(h))
    return score


def distmult_score_backward(h, w, s, r, o, grad_score, plan: TriplePlan, want_h: bool = True, want_w: bool = True):
    """(grad_h [N, D] in h's dtype or None, grad_w [R, D] fp32 or None) of het_distmult_score_backward / _bf16 for ``grad_score`` [T] fp32
    and the batch's ``plan`` (triple_plan): node-major and relation-major sums in a fixed order, every row written once."""
    _distmult_chk("distmult_score_backward", h, w, s, r, o)
    _chk("distmult_score_backward", (grad_score,), tuple(plan[:6]))
    T, N, R = s.shape[0], h.shape[0], w.shape[0]
    if (grad_score.shape != (T,) or grad_score.device != h.device or (plan.num_nodes, plan.num_rels) != (N, R)
            or plan.node_ptr.shape != (N + 1,) or plan.node_slots.shape != (2 * T,) or plan.rel_ptr.shape != (R + 1,)
            or plan.rel_order.shape != (T,) or plan.chunk_ptr.shape != (N + R + 2,) or any(t.device != h.device for t in plan[:6])):
        raise _lib.HetError(f"distmult_score_backward: grad_score [{T}] and the plan of these {T} triples over {N} nodes and {R} relations on "
                            f"{h.device} expected, got {tuple(grad_score.shape)} and a plan for {plan.num_nodes} nodes, {plan.num_rels} "
                            f"relations, {plan.rel_order.shape[0]} triples")
    return _distmult_score_backward(h, w, s, r, o, grad_score, plan, want_h, want_w)


def _distmult_score_backward(h, w, s, r, o, grad_score, plan, want_h, want_w):
    T, (N, D), R = s.shape[0], h.shape, w.shape[0]
    grad_h = torch.empty_like(h) if want_h else None
    grad_w = torch.empty_like(w) if want_w else None
    if not (want_h or want_w):
        return None, None
    ws, nbytes = _workspace(h, "het_distmult_score_backward_workspace", T, R, D)
    _call(h, "het_distmult_score_backward_bf16" if h.dtype == torch.bfloat16 else "het_distmult_score_backward", _p(h), _p(w), _p(s), _p(r),
          _p(o), _p(grad_score), _p(plan.node_ptr), _p(plan.node_slots), _p(plan.rel_ptr), _p(plan.rel_order), _p(plan.chunk_ptr), T, N, R, D,
          _p(grad_h), _p(grad_w), _p(ws), nbytes, _stream(h))
    return grad_h, grad_w


# ---- filtered ranking of link-prediction queries (het_amd/linkpred.py distmult_rank; csrc/triple_rank.hip) ----
_TRIPLE_RANK_PARAMS = ("query_tile", "cand_tile", "min_width", "max_width", "block", "max_blocks", "chunk_tiles", "max_span")


def triple_rank_params() -> Dict[str, int]:
    """The launch constants of csrc/triple_rank.hip (het_triple_rank_params; runs on the host): a workgroup multiplies tiles of
    ``query_tile`` queries by ``cand_tile`` candidates; the widths D served are the multiples of 4 from ``min_width`` to ``max_width``;
    ``block`` threads per workgroup, at most ``max_blocks`` workgroups; a workgroup keeps the counters of ``chunk_tiles`` query tiles
    and takes at most ``max_span`` candidate tiles per work item."""
    L = _lib.lib()
    out = (C.c_int64 * len(_TRIPLE_RANK_PARAMS))()
    rc = L.het_triple_rank_params(out)
    if rc != 0:
        raise _lib.HetError(f"het_triple_rank_params failed (code {rc}): {L.het_last_error().decode()}")
    return dict(zip(_TRIPLE_RANK_PARAMS, (int(v) for v in out)))


def triple_rank_ok(h, w) -> bool:
    """Whether het_triple_rank takes these tables: h [N, D] contiguous float32 / bfloat16 on a GPU, 16-byte (bf16: 8-byte) aligned, w
    [R, D] contiguous float32 on the same device, D a width of triple_rank_params(), N and R below 2^31 - 1."""
    p = triple_rank_params()
    return (h.is_cuda and h.dim() == 2 and w.dim() == 2 and h.dtype in (torch.float32, torch.bfloat16) and w.dtype == torch.float32
            and w.device == h.device and h.shape[1] == w.shape[1] and h.is_contiguous() and w.is_contiguous()
            and h.data_ptr() % (4 * h.element_size()) == 0 and w.data_ptr() % 16 == 0
            and p["min_width"] <= h.shape[1] <= p["max_width"] and h.shape[1] % 4 == 0
            and h.shape[0] < 2 ** 31 - 1 and w.shape[0] < 2 ** 31 - 1)


def triple_rank(h, w, anchor, rel, truth, pair_query=None, pair_cand=None, node_type_offsets=None):
    """(greater, equal, cands) int32 [Q] and bad int64 [1] of het_triple_rank / _bf16: every query (anchor, rel, truth) ranked against
    the nodes of its true node's run with the DistMult score (the rule in include/het_amd.h), the listed (pair_query, pair_cand) pairs
    and the true node excluded.  ``node_type_offsets``: an int64 tensor on h's device, or None.  Nothing is read back."""
    if not triple_rank_ok(h, w):
        raise _lib.HetError(f"triple_rank: expected contiguous float32 or bfloat16 GPU rows h [N, D], 16-byte (bf16: 8-byte) aligned, and "
                            f"float32 w [R, D] on the same device with D a multiple of 4 in the widths of triple_rank_params(), got {h.dtype} "
                            f"{tuple(h.shape)} on {h.device}{'' if h.is_contiguous() else ' (non-contiguous)'} and {w.dtype} "
                            f"{tuple(w.shape)} on {w.device}")
    _triple_ids_chk("triple_rank", h, anchor, rel, truth)
    if (pair_query is None) != (pair_cand is None):
        raise _lib.HetError("triple_rank: pair_query and pair_cand come together")
    NP = 0
    if pair_query is not None:
        _triple_ids_chk("triple_rank", h, pair_query, pair_cand)
        NP = pair_query.shape[0]
    offs, ntypes = None, 0
    if node_type_offsets is not None:
        offs = node_type_offsets
        if not (offs.is_cuda and offs.device == h.device and offs.dtype == torch.int64 and offs.dim() == 1 and offs.numel() >= 2
                and offs.is_contiguous()):
            raise _lib.HetError(f"triple_rank: node_type_offsets is a contiguous int64 tensor [num_types + 1] on {h.device}, got "
                                f"{offs.dtype} {tuple(offs.shape)} on {offs.device}")
        ntypes = offs.numel() - 1
    Q, (N, D), R = anchor.shape[0], h.shape, w.shape[0]
    out = torch.empty(3, Q, dtype=torch.int32, device=h.device)
    bad = torch.empty(1, dtype=torch.int64, device=h.device)
    if Q == 0:
        return out[0], out[1], out[2], bad.zero_()
    ws, nbytes = _workspace(h, "het_triple_rank_workspace", Q, NP, N, D)
    _call(h, "het_triple_rank_bf16" if h.dtype == torch.bfloat16 else "het_triple_rank", _p(h), _p(w), _p(anchor), _p(rel), _p(truth), Q,
          _p(pair_query) if NP else None, _p(pair_cand) if NP else None, NP, _p(offs), ntypes, N, R, D, _p(out[0]), _p(out[1]), _p(out[2]),
          _p(bad), _p(ws), nbytes, _stream(h))
    return out[0], out[1], out[2], bad


# ---- the ComplEx head (het_amd/linkpred.py ComplExDecoder, complex_rank; csrc/triple_score.hip, csrc/triple_rank.hip) ----
def complex_ok(h, w) -> bool:
    """Whether the ComplEx score kernels take these tables: what ``distmult_ok`` asks (a width of triple_params() is a multiple of 4,
    so every 16-byte piece of a row holds two whole complex numbers: column 2k the real, 2k + 1 the imaginary part)."""
    return distmult_ok(h, w)


def _complex_chk(name, h, w, s, r, o):
    if not complex_ok(h, w):
        raise _lib.HetError(f"{name}: expected contiguous float32 or bfloat16 GPU rows h [N, D], 16-byte (bf16: 8-byte) aligned, and float32 "
                            f"w [R, D] on the same device with D a multiple of 4 in the widths of triple_params(), got {h.dtype} "
                            f"{tuple(h.shape)} on {h.device}{'' if h.is_contiguous() else ' (non-contiguous)'} and {w.dtype} {tuple(w.shape)} "
                            f"on {w.device}")
    _triple_ids_chk(name, h, s, r, o)


def complex_score(h, w, s, r, o):
    """score [T] fp32 = sum_k Re(h[s]_k * w[r]_k * conj(h[o]_k)) over the D / 2 complex components of the rows (het_complex_score /
    _bf16; one launch); +0 for a triple with an id outside its table."""
    _complex_chk("complex_score", h, w, s, r, o)
    return _complex_score(h, w, s, r, o)


def _complex_score(h, w, s, r, o):
    T = s.shape[0]
    score = torch.empty(T, dtype=torch.float32, device=h.device)
    if T:
        _call(h, "het_complex_score_bf16" if h.dtype == torch.bfloat16 else "het_complex_score", _p(h), _p(w), _p(s), _p(r), _p(o), T,
              h.shape[0], w.shape[0], h.shape[1], _p(score), _stream(h))
    return score


def complex_score_backward(h, w, s, r, o, grad_score, plan: TriplePlan, want_h: bool = True, want_w: bool = True):
    """(grad_h [N, D] in h's dtype or None, grad_w [R, D] fp32 or None) of het_complex_score_backward / _bf16 for ``grad_score`` [T] fp32
    and the batch's ``plan`` (triple_plan, the one the DistMult head uses): the same lists, chunks and orders."""
    _complex_chk("complex_score_backward", h, w, s, r, o)
    _chk("complex_score_backward", (grad_score,), tuple(plan[:6]))
    T, N, R = s.shape[0], h.shape[0], w.shape[0]
    if (grad_score.shape != (T,) or grad_score.device != h.device or (plan.num_nodes, plan.num_rels) != (N, R)
            or plan.node_ptr.shape != (N + 1,) or plan.node_slots.shape != (2 * T,) or plan.rel_ptr.shape != (R + 1,)
            or plan.rel_order.shape != (T,) or plan.chunk_ptr.shape != (N + R + 2,) or any(t.device != h.device for t in plan[:6])):
        raise _lib.HetError(f"complex_score_backward: grad_score [{T}] and the plan of these {T} triples over {N} nodes and {R} relations on "
                            f"{h.device} expected, got {tuple(grad_score.shape)} and a plan for {plan.num_nodes} nodes, {plan.num_rels} "
                            f"relations, {plan.rel_order.shape[0]} triples")
    return _complex_score_backward(h, w, s, r, o, grad_score, plan, want_h, want_w)


def _complex_score_backward(h, w, s, r, o, grad_score, plan, want_h, want_w):
    T, (N, D), R = s.shape[0], h.shape, w.shape[0]
    grad_h = torch.empty_like(h) if want_h else None
    grad_w = torch.empty_like(w) if want_w else None
    if not (want_h or want_w):
        return None, None
    ws, nbytes = _workspace(h, "het_distmult_score_backward_workspace", T, R, D)
    _call(h, "het_complex_score_backward_bf16" if h.dtype == torch.bfloat16 else "het_complex_score_backward", _p(h), _p(w), _p(s), _p(r),
          _p(o), _p(grad_score), _p(plan.node_ptr), _p(plan.node_slots), _p(plan.rel_ptr), _p(plan.rel_order), _p(plan.chunk_ptr), T, N, R, D,
          _p(grad_h), _p(grad_w), _p(ws), nbytes, _stream(h))
    return grad_h, grad_w


def complex_rank(h, w, anchor, rel, truth, side, pair_query=None, pair_cand=None, node_type_offsets=None):
    """(greater, equal, cands) int32 [Q] and bad int64 [1] of het_complex_rank / _bf16: ``triple_rank`` with the ComplEx score (the rule
    in include/het_amd.h).  ``side`` [Q] int64: 0 ranks tails (the anchor is the head), 1 ranks heads (the anchor is the tail); any
    other value makes the query bad.  Nothing is read back."""
    if not triple_rank_ok(h, w):
        raise _lib.HetError(f"complex_rank: expected contiguous float32 or bfloat16 GPU rows h [N, D], 16-byte (bf16: 8-byte) aligned, and "
                            f"float32 w [R, D] on the same device with D a multiple of 4 in the widths of triple_rank_params(), got {h.dtype} "
                            f"{tuple(h.shape)} on {h.device}{'' if h.is_contiguous() else ' (non-contiguous)'} and {w.dtype} "
                            f"{tuple(w.shape)} on {w.device}")
    _triple_ids_chk("complex_rank", h, anchor, rel, truth, side)
    if (pair_query is None) != (pair_cand is None):
        raise _lib.HetError("complex_rank: pair_query and pair_cand come together")
    NP = 0
    if pair_query is not None:
        _triple_ids_chk("complex_rank", h, pair_query, pair_cand)
        NP = pair_query.shape[0]
    offs, ntypes = None, 0
    if node_type_offsets is not None:
        offs = node_type_offsets
        if not (offs.is_cuda and offs.device == h.device and offs.dtype == torch.int64 and offs.dim() == 1 and offs.numel() >= 2
                and offs.is_contiguous()):
            raise _lib.HetError(f"complex_rank: node_type_offsets is a contiguous int64 tensor [num_types + 1] on {h.device}, got "
                                f"{offs.dtype} {tuple(offs.shape)} on {offs.device}")
        ntypes = offs.numel() - 1
    Q, (N, D), R = anchor.shape[0], h.shape, w.shape[0]
    out = torch.empty(3, Q, dtype=torch.int32, device=h.device)
    bad = torch.empty(1, dtype=torch.int64, device=h.device)
    if Q == 0:
        return out[0], out[1], out[2], bad.zero_()
    ws, nbytes = _workspace(h, "het_triple_rank_workspace", Q, NP, N, D)
    _call(h, "het_complex_rank_bf16" if h.dtype == torch.bfloat16 else "het_complex_rank", _p(h), _p(w), _p(anchor), _p(rel), _p(truth),
          _p(side), Q, _p(pair_query) if NP else None, _p(pair_cand) if NP else None, NP, _p(offs), ntypes, N, R, D, _p(out[0]), _p(out[1]),
          _p(out[2]), _p(bad), _p(ws), nbytes, _stream(h))
    return out[0], out[1], out[2], bad


def rgat_backward_compact(groupings, feat_c, el_c, er_c, sum, ret, gradout, grad_feat_c, grad_el_c, grad_er_c, slope,
                          fold_attn_l=None, row_rel_ptrs=None, grad_bias=None, bias_rows=0, runs=None, drow_nodes=None,
                          grad_attn_l=None, finish_attn_grad=True):
    """runs = (q_rows, q_sum, q_ref) of rgat_aggregate_compact in the run-sum form, drow_nodes [S_col] int64 the destination of
    every er row: grad_er_c from the run sums (het_rgat_backward_compact_runs).  grad_attn_l [R,H,D] (run-sum form, with
    fold_attn_l): also the weight gradient of el_c = <feat_c, attn_l[r]>, from the same pass.
    ``finish_attn_grad=False`` (with grad_attn_l): the edge pass alone (het_rgat_backward_compact_runs_edges) -- grad_attn_l's partial
    rows stay in the workspace, and what is returned goes to rgat_attn_grad_finish, on this stream or on one that waits for it.  The
    returned tuple holds the workspace: keep it until the finishing launch is ordered before whatever allocates next."""
    _chk("rgat_backward_compact", tuple(t for t in (feat_c, el_c, er_c, sum, ret, gradout, grad_feat_c, grad_el_c, grad_er_c,
                                                    fold_attn_l, grad_bias, grad_attn_l) + (tuple(runs) if runs else ()) if t is not None),
         tuple(t for t in (row_rel_ptrs, drow_nodes) if t is not None))
    return _rgat_backward_compact("het_rgat_backward_compact_runs%s", groupings, feat_c, el_c, er_c, sum, ret, gradout, grad_feat_c,
                                  grad_el_c, grad_er_c, slope, fold_attn_l, row_rel_ptrs, grad_bias, bias_rows, runs, drow_nodes, grad_attn_l,
                                  finish_attn_grad)


def _rgat_backward_compact(runs_entry, groupings, feat_c, el_c, er_c, sum, ret, gradout, grad_feat_c, grad_el_c, grad_er_c, slope,
                           fold_attn_l, row_rel_ptrs, grad_bias, bias_rows, runs, drow_nodes, grad_attn_l, finish_attn_grad=True):
    """rgat_backward_compact / _bf16 behind their tensor checks; ``runs_entry``: the C entry of the run-sum form, with a %s where its
    first half has "_edges".  Returns what rgat_attn_grad_finish takes when the finishing pass is left to the caller, else None."""
    split = bool(runs) and grad_attn_l is not None and not finish_attn_grad
    runs_entry = runs_entry % ("_edges" if split else "")
    N, H = sum.shape[0], sum.shape[1]
    D = ret.numel() // max(1, N * H)
    if runs and row_rel_ptrs is not None:
        groupings[1].pin_key(runs_entry, row_rel_ptrs)
    if runs:
        ws, nbytes = _workspace(ret, "het_rgat_backward_compact_runs_workspace", groupings[1].handle, N, er_c.shape[0], H, D,
                                int(grad_bias is not None), int(grad_attn_l is not None), _stream(ret))
    else:
        assert grad_attn_l is None, "grad_attn_l comes with the run-sum form"
        ws, nbytes = _workspace(ret, "het_rgat_backward_compact_workspace", N, groupings[1]._keep[1].numel(), H, D,
                                int(grad_bias is not None))
    head = (_p(feat_c), _p(el_c), _p(er_c), _p(sum), _p(ret), _p(gradout), _p(grad_feat_c), _p(grad_el_c), _p(grad_er_c),
            _p(fold_attn_l), _p(row_rel_ptrs), 0 if row_rel_ptrs is None else row_rel_ptrs.numel() - 1, _p(grad_bias),
            int(bias_rows), N, feat_c.shape[0], er_c.shape[0], H, D, float(slope))
    tail = (_p(ws), nbytes, _stream(ret))
    if runs:
        _call(ret, runs_entry, groupings[1].handle, _p(runs[0]), _p(runs[1]), _p(runs[2]), _p(drow_nodes), *head,
              _p(grad_attn_l), *tail)
        if split:
            return (groupings[1], N, er_c.shape[0], row_rel_ptrs.numel() - 1, H, D, int(grad_bias is not None), grad_attn_l, ws, nbytes)
    else:
        _call(ret, "het_rgat_backward_compact", groupings[1].handle, groupings[2].handle, *head, *tail)


def rgat_attn_grad_finish(pending):
    """The second half of rgat_backward_compact(..., finish_attn_grad=False), on the current stream (het_rgat_attn_grad_finish):
    grad_attn_l += the partial rows the edge pass left in its workspace."""
    by_srow, N, S_col, R, H, D, with_bias, grad_attn_l, ws, nbytes = pending
    _call(grad_attn_l, "het_rgat_attn_grad_finish", by_srow.handle, N, S_col, R, H, D, with_bias, _p(grad_attn_l), _p(ws), nbytes,
          _stream(grad_attn_l))


def rgat_transpose_weights(W, loop_w=None):
    """(W^T [R,H,D,K], loop_w^T [X,K] or None) of W [R,H,K,D] and loop_w [K,X] in one launch (het_rgat_transpose_weights): exact
    copies, what transpose(...).contiguous() gives."""
    _chk("rgat_transpose_weights", (W,) if loop_w is None else (W, loop_w))
    R, H, Kd, D = W.shape
    if loop_w is not None and (loop_w.dim() != 2 or loop_w.shape[0] != Kd):
        raise _lib.HetError(f"rgat_transpose_weights: loop_w {tuple(loop_w.shape)} does not fit W {tuple(W.shape)}")
    Wt = torch.empty((R, H, D, Kd), dtype=W.dtype, device=W.device)
    X = 0 if loop_w is None else loop_w.shape[1]
    loop_wt = None if loop_w is None else torch.empty((X, Kd), dtype=W.dtype, device=W.device)
    _call(W, "het_rgat_transpose_weights", _p(W), R, H, Kd, D, _p(Wt), _p(loop_w), X, _p(loop_wt), _stream(W))
    return Wt, loop_wt


def rgat_unfold_weight_gradient(grad_wa, W, attn_r, grad_W):
    """The gradient through wa = W . attn_r in one launch (het_rgat_unfold_weight_gradient): grad_W [R,H,K,D] += grad_wa (x) attn_r in
    place; returns grad_attn_r [R,H,D].  grad_wa: R*H*K floats ([R,H,K,1] or [R,H,K])."""
    _chk("rgat_unfold_weight_gradient", (grad_wa, W, attn_r, grad_W))
    R, H, Kd, D = W.shape
    if grad_wa.numel() != R * H * Kd or attn_r.numel() != R * H * D or grad_W.shape != W.shape:
        raise _lib.HetError(f"rgat_unfold_weight_gradient: grad_wa {tuple(grad_wa.shape)}, attn_r {tuple(attn_r.shape)} and grad_W "
                            f"{tuple(grad_W.shape)} do not fit W {tuple(W.shape)}")
    grad_attn_r = torch.empty((R, H, D), dtype=W.dtype, device=W.device)
    torch.autograd.graph.increment_version(grad_W)
    _call(W, "het_rgat_unfold_weight_gradient", _p(grad_wa), _p(W), _p(attn_r), R, H, Kd, D, _p(grad_W), _p(grad_attn_r), _stream(W))
    return grad_attn_r


def hgt_fold_source_weights(k_lin, v_lin, rel_att, rel_msg, rel_pri, src_type, transpose_att: bool):
    """w_kv [R,1,in,2*H*dk] (include/het_amd.h: het_hgt_fold_source_weights).  k_lin / v_lin [T,1,in,H*dk] contiguous fp32 on the GPU."""
    _chk("hgt_fold_source_weights", (k_lin, v_lin, rel_att, rel_msg, rel_pri), (src_type,))
    R, H, dk, _ = rel_att.shape
    T, K_in = k_lin.shape[0], k_lin.shape[2]
    w = torch.empty((R, 1, K_in, 2 * H * dk), dtype=k_lin.dtype, device=k_lin.device)
    _call(w, "het_hgt_fold_source_weights", _p(k_lin), _p(v_lin), _p(rel_att), _p(rel_msg), _p(rel_pri), _p(src_type), T, R, H, dk, K_in,
          int(transpose_att), _p(w), _stream(w))
    return w


def hgt_fold_source_weights_backward(grad_w, k_lin, v_lin, rel_att, rel_msg, rel_pri, src_type, transpose_att: bool):
    """(grad_k_lin, grad_v_lin, grad_att, grad_msg, grad_pri) of hgt_fold_source_weights."""
    _chk("hgt_fold_source_weights_backward", (grad_w, k_lin, v_lin, rel_att, rel_msg, rel_pri), (src_type,))
    R, H, dk, _ = rel_att.shape
    T, K_in = k_lin.shape[0], k_lin.shape[2]
    outs = tuple(torch.empty_like(t) for t in (k_lin, v_lin, rel_att, rel_msg, rel_pri))
    _call(grad_w, "het_hgt_fold_source_weights_backward", _p(grad_w), _p(k_lin), _p(v_lin), _p(rel_att), _p(rel_msg), _p(rel_pri),
          _p(src_type), T, R, H, dk, K_in, int(transpose_att), *(_p(o) for o in outs), _stream(grad_w))
    return outs


def hgt_compact_shape_ok(H: int, D: int) -> bool:
    return bool(_lib.lib().het_hgt_compact_shape_ok(int(H), int(D)))


def destination_lists(col, offsets):
    """(dst_nodes [S_dst] sorted, rank_of_edge [E], run_ptrs [len(offsets)]) for the destinations that HAVE in-edges: the
    distinct values of ``col``, the index of every edge's destination in that list, and the list split at the node-type
    offsets (rows of a node type are a contiguous piece of the sorted list).  Built once per graph (cached)."""
    def build():
        nodes, inv = torch.unique(col, return_inverse=True)
        ptrs = torch.searchsorted(nodes, offsets.to(nodes.dtype)).contiguous()
        return nodes.contiguous(), inv.contiguous(), ptrs
    return _derived_get("dst_lists", (col, offsets), build)


def hgt_compact_groupings(col, srow, num_nodes, num_src_rows):
    """The two groupings of the compact HGT passes (include/het_amd.h: het_hgt_aggregate_compact): by destination and by
    (relation, source) row.  ``srow`` [E] int64: that row of every edge position."""
    by_dst = _plan.get_grouping(None, col, num_nodes, srow, None)
    by_srow = _plan.get_grouping(None, srow, num_src_rows, col, None)
    return None if by_dst is None or by_srow is None else (by_dst, by_srow)


def _hgt_aggregate_compact(entry, groupings, kv_c, q, lsum, out, workspace=None):
    """hgt_aggregate_compact / _bf16 behind their tensor checks (``workspace``: the caller's buffer instead of one sized by the query)."""
    N, H = lsum.shape
    D = out.numel() // max(1, N * H)
    if workspace is None:
        ws, nbytes = _workspace(out, "het_hgt_aggregate_compact_workspace", groupings[0].handle, H, D)  # (hub destinations only)
    else:
        ws, nbytes = workspace, workspace.numel() * 4
    _call(out, entry, groupings[0].handle, _p(kv_c), _p(q), _p(lsum), _p(out), N, kv_c.shape[0], H, D, _p(ws), nbytes, _stream(out))


def _hgt_backward_compact(entry, groupings, kv_c, q, lsum, out, gradout, grad_kv_c, grad_q, workspace=None):
    """hgt_backward_compact / _bf16 behind their tensor checks."""
    N, H = lsum.shape
    D = out.numel() // max(1, N * H)
    if workspace is None:
        ws, nbytes = _workspace(out, "het_hgt_backward_compact_workspace", N, H)
    else:
        ws, nbytes = workspace, workspace.numel() * 4
    _call(out, entry, groupings[0].handle, groupings[1].handle, _p(kv_c), _p(q), _p(lsum), _p(out), _p(gradout), _p(grad_kv_c),
          _p(grad_q), N, kv_c.shape[0], H, D, _p(ws), nbytes, _stream(out))


def hgt_aggregate_compact(groupings, kv_c, q, lsum, out):
    _chk("hgt_aggregate_compact", (kv_c, q, lsum, out))
    _hgt_aggregate_compact("het_hgt_aggregate_compact", groupings, kv_c, q, lsum, out)


def hgt_backward_compact(groupings, kv_c, q, lsum, out, gradout, grad_kv_c, grad_q):
    _chk("hgt_backward_compact", (kv_c, q, lsum, out, gradout, grad_kv_c, grad_q))
    _hgt_backward_compact("het_hgt_backward_compact", groupings, kv_c, q, lsum, out, gradout, grad_kv_c, grad_q)


def gat_rank_of_position(rel_ptrs, row, col, eids, num_nodes):
    """[E] int64: the rank of every separate-COO position in the destination-grouped order of the kind-0 GAT kernels
    (row j of exp_sorted / grad_el_sorted belongs to the position whose rank is j).  None without groupings."""
    g = _by_dst(0, (None, None, None, None), rel_ptrs, row, col, eids, num_nodes)
    if g is None:
        return None
    r = getattr(g, "rank_of_position", None)
    if r is None:
        with _plan.building():  # (kept with the grouping: a normal tensor whatever the caller's mode)
            r = torch.empty(eids.numel(), dtype=torch.int64, device=eids.device)
        _call(r, "het_grouping_rank_of_position", g.handle, _p(r), _stream(r))
        g.rank_of_position = r  # lives (and is evicted) with the grouping
    return r


@_op("relational_fused_gat_csr(Tensor incsr_row_ptr, Tensor incsr_col_indices, Tensor incsr_eids, Tensor incsr_reltypes, "
     "Tensor unique_srcs_and_dests_rel_ptrs, Tensor unique_srcs_and_dests_node_indices, Tensor feat_src, Tensor el, "
     "Tensor er, Tensor(a!) sum, Tensor(b!) exp, Tensor(c!) ret, float slope, bool CompactAsOfNodeFlag=False) -> ()")
def relational_fused_gat_csr(incsr_row_ptr, incsr_col_indices, incsr_eids, incsr_reltypes,
                             unique_srcs_and_dests_rel_ptrs, unique_srcs_and_dests_node_indices, feat_src, el, er, sum,
                             exp, ret, slope, CompactAsOfNodeFlag=False):
    _chk("relational_fused_gat_csr", (feat_src, el, er, sum, exp, ret),
         (incsr_row_ptr, incsr_col_indices, incsr_eids, incsr_reltypes))
    N, E, H = incsr_row_ptr.numel() - 1, incsr_eids.numel(), el.shape[1]
    D = ret.numel() // max(1, N * H)
    if not CompactAsOfNodeFlag and _plan.is_enabled() and E > 0 and gat_grouped_shape_ok(H, D):
        # the in-CSR IS the edge list grouped by destination: same math as the separate-COO op on (eids, src, dst) in
        # CSR order, served by the destination-grouped kernels instead of E*H*D float atomics
        dst, rp1 = _csr_expanded_rows(incsr_row_ptr, E)
        fused_gat_forward(incsr_eids, rp1, incsr_col_indices, dst, 0, {}, feat_src, el, er, sum, exp, ret, slope, None)
        return
    if CompactAsOfNodeFlag and _plan.is_enabled() and E > 0 and gat_grouped_shape_ok(H, D):
        # compact rows: the same op as the separate-COO pair with CompactAsOfNodeKind 4 once every edge id knows its feat
        # row and er row (cached per graph) -- destination-grouped kernels instead of float atomics
        dst, maps = _csr_compact_maps(incsr_row_ptr, incsr_col_indices, incsr_eids, incsr_reltypes,
                                      unique_srcs_and_dests_rel_ptrs, unique_srcs_and_dests_node_indices, True)
        _, rp1 = _csr_expanded_rows(incsr_row_ptr, E)
        fused_gat_forward(incsr_eids, rp1, incsr_col_indices, dst, 4, maps, feat_src, el, er, sum, exp, ret, slope, None)
        return
    _call(ret, "het_relational_fused_gat_csr", _p(incsr_row_ptr), _p(incsr_col_indices), _p(incsr_eids),
          _p(incsr_reltypes), N, E, _p(unique_srcs_and_dests_rel_ptrs), _p(unique_srcs_and_dests_node_indices),
          max(0, unique_srcs_and_dests_rel_ptrs.numel() - 1), _p(feat_src), _p(el), _p(er), _p(sum), _p(exp), _p(ret),
          H, D, float(slope), int(CompactAsOfNodeFlag), _stream(ret))


@_op("backward_relational_fused_gat_csr(Tensor outcsr_row_ptr, Tensor outcsr_col_indices, Tensor outcsr_eids, "
     "Tensor outcsr_reltypes, Tensor unique_srcs_and_dests_rel_ptrs, Tensor unique_srcs_and_dests_node_indices, "
     "Tensor feat_src, Tensor el, Tensor er, Tensor sum, Tensor exp, Tensor ret, Tensor gradout, "
     "Tensor(a!) grad_feat_src, Tensor(b!) grad_el, Tensor(c!) grad_er, float slope, bool CompactAsOfNodeFlag=False) -> ()")
def backward_relational_fused_gat_csr(outcsr_row_ptr, outcsr_col_indices, outcsr_eids, outcsr_reltypes,
                                      unique_srcs_and_dests_rel_ptrs, unique_srcs_and_dests_node_indices, feat_src, el,
                                      er, sum, exp, ret, gradout, grad_feat_src, grad_el, grad_er, slope,
                                      CompactAsOfNodeFlag=False):
    _chk("backward_relational_fused_gat_csr", (feat_src, el, er, sum, exp, ret, gradout, grad_feat_src, grad_el, grad_er),
         (outcsr_row_ptr, outcsr_col_indices, outcsr_eids, outcsr_reltypes))
    N, E, H = outcsr_row_ptr.numel() - 1, outcsr_eids.numel(), el.shape[1]
    D = ret.numel() // max(1, N * H)
    if not CompactAsOfNodeFlag and _plan.is_enabled() and E > 0 and gat_grouped_shape_ok(H, D) and slope >= 0:
        # out-CSR rows are the sources: (eids, src, dst) in CSR order through the destination-grouped backward (every
        # gradient row of kind 0 belongs to one edge, so "+=" into the zero-filled buffers equals the stores it does)
        src, rp1 = _csr_expanded_rows(outcsr_row_ptr, E)
        fused_gat_backward(outcsr_eids, rp1, src, outcsr_col_indices, 0, {}, feat_src, el, er, sum, exp, ret, gradout,
                           grad_feat_src, grad_el, grad_er, slope, None)
        return
    if CompactAsOfNodeFlag and _plan.is_enabled() and E > 0 and gat_grouped_shape_ok(H, D) and slope >= 0:
        src, maps = _csr_compact_maps(outcsr_row_ptr, outcsr_col_indices, outcsr_eids, outcsr_reltypes,
                                      unique_srcs_and_dests_rel_ptrs, unique_srcs_and_dests_node_indices, False)
        _, rp1 = _csr_expanded_rows(outcsr_row_ptr, E)
        # "+=" contract of the reference-named op: the kind-4 kernels overwrite, so they run into temporaries that are added
        gf, gl, gr = torch.zeros_like(grad_feat_src), torch.zeros_like(grad_el), torch.zeros_like(grad_er)
        fused_gat_backward(outcsr_eids, rp1, src, outcsr_col_indices, 4, maps, feat_src, el, er, sum, exp, ret, gradout,
                           gf, gl, gr, slope, None)
        grad_feat_src += gf
        grad_el += gl
        grad_er += gr
        return
    _call(ret, "het_backward_relational_fused_gat_csr", _p(outcsr_row_ptr), _p(outcsr_col_indices), _p(outcsr_eids),
          _p(outcsr_reltypes), N, E, _p(unique_srcs_and_dests_rel_ptrs), _p(unique_srcs_and_dests_node_indices),
          max(0, unique_srcs_and_dests_rel_ptrs.numel() - 1), _p(feat_src), _p(el), _p(er), _p(sum), _p(exp), _p(ret),
          _p(gradout), _p(grad_feat_src), _p(grad_el), _p(grad_er), H, D, float(slope), int(CompactAsOfNodeFlag),
          _stream(ret))


# ------------------------------------------------------------------------------------
# RGCN
# ------------------------------------------------------------------------------------
@_op("rgcn_layer1_separate_coo(Tensor separate_coo_relptrs, Tensor separate_coo_eids, Tensor separate_coo_row_indices, "
     "Tensor separate_coo_col_indices, Tensor node_feat_input, Tensor weights, Tensor edge_norm, "
     "Tensor(a!) node_feat_output) -> ()")
def rgcn_layer1_separate_coo(separate_coo_relptrs, separate_coo_eids, separate_coo_row_indices,
                             separate_coo_col_indices, node_feat_input, weights, edge_norm, node_feat_output):
    _chk("rgcn_layer1_separate_coo", (node_feat_input, weights, edge_norm, node_feat_output),
         (separate_coo_relptrs, separate_coo_eids, separate_coo_row_indices, separate_coo_col_indices))
    R, K, D = weights.shape
    N = node_feat_output.shape[0]
    g = _plan.get_grouping(separate_coo_relptrs, separate_coo_col_indices, N, separate_coo_row_indices, separate_coo_eids)
    ws = None if g is None else torch.empty(max(1, g.num_segments) * K, dtype=torch.float32, device=weights.device)
    _call(node_feat_output, "het_rgcn_layer1_separate_coo", _p(separate_coo_relptrs), _p(separate_coo_eids),
          _p(separate_coo_row_indices), _p(separate_coo_col_indices), R, separate_coo_eids.numel(), N,
          _p(node_feat_input), _p(weights), _p(edge_norm), _p(node_feat_output), K, D, None if g is None else g.handle,
          _p(ws), 0 if ws is None else ws.numel() * 4, _stream(node_feat_output))


@_op("backward_rgcn_layer1_separate_coo(Tensor separate_coo_relptrs, Tensor separate_coo_eids, "
     "Tensor separate_coo_row_indices, Tensor separate_coo_col_indices, Tensor node_feat_input, "
     "Tensor weights_transposed, Tensor edge_norm, Tensor(a!) grad_edge_norm, Tensor(b!) delta_node_feat_input, "
     "Tensor delta_node_feat_output, Tensor(c!) delta_weights) -> ()")
def backward_rgcn_layer1_separate_coo(separate_coo_relptrs, separate_coo_eids, separate_coo_row_indices,
                                      separate_coo_col_indices, node_feat_input, weights_transposed, edge_norm,
                                      grad_edge_norm, delta_node_feat_input, delta_node_feat_output, delta_weights):
    _chk("backward_rgcn_layer1_separate_coo",
         (node_feat_input, weights_transposed, edge_norm, delta_node_feat_input, delta_node_feat_output, delta_weights),
         (separate_coo_relptrs, separate_coo_eids, separate_coo_row_indices, separate_coo_col_indices))
    R, D, K = weights_transposed.shape
    N = delta_node_feat_output.shape[0]
    g = _plan.get_grouping(separate_coo_relptrs, separate_coo_row_indices, node_feat_input.shape[0],
                           separate_coo_col_indices, separate_coo_eids)
    ws = None if g is None else torch.empty(max(1, g.num_segments) * D, dtype=torch.float32, device=delta_weights.device)
    _call(delta_weights, "het_backward_rgcn_layer1_separate_coo", _p(separate_coo_relptrs), _p(separate_coo_eids),
          _p(separate_coo_row_indices), _p(separate_coo_col_indices), R, separate_coo_eids.numel(), N,
          _p(node_feat_input), _p(weights_transposed), _p(edge_norm), _p(grad_edge_norm), _p(delta_node_feat_input),
          _p(delta_node_feat_output), _p(delta_weights), K, D, None if g is None else g.handle, _p(ws),
          0 if ws is None else ws.numel() * 4, _stream(delta_weights))


def rgcn_layer_ok(R: int, K: int, D: int) -> bool:
    """Shapes of the two-call RGCN layer (include/het_amd.h: het_rgcn_layer_forward)."""
    return bool(_lib.lib().het_rgcn_layer_ok(int(R), int(K), int(D)))


def _grouping_segment_map(g, rel_ptrs, keys, num_keys: int):
    """[R, num_keys] int32: segment of (relation, key) in the grouping ``g`` of ``keys`` by (relation, key), -1 = none (cached by
    the identity of the lists the grouping was built from)."""
    def build():
        R = rel_ptrs.numel() - 1
        m = torch.empty((R, num_keys), dtype=torch.int32, device=keys.device)
        _call(keys, "het_grouping_segment_map", g.handle, num_keys, _p(m), _stream(keys))
        return m
    return _derived_get(("segmap", num_keys), (rel_ptrs, keys), build)


def rgcn_layer_plan(rel_ptrs, eids, row, col, num_nodes: int):
    """What the two-call RGCN layer needs per graph (groupings from het_amd.plan, the rest cached by tensor identity):
    (by_rel_dst, by_rel_src, dst_map, dst_order, src_map, src_order), or None without groupings.  The maps come from the
    groupings' own segment lists, so a graph needs no unique (relation, node) lists for this layer."""
    gd = _plan.get_grouping(rel_ptrs, col, num_nodes, row, eids)
    gs = _plan.get_grouping(rel_ptrs, row, num_nodes, col, eids)
    if gd is None or gs is None:
        return None
    dst_map = _grouping_segment_map(gd, rel_ptrs, col, num_nodes)
    src_map = _grouping_segment_map(gs, rel_ptrs, row, num_nodes)
    return gd, gs, dst_map, node_order_by_presence(dst_map), src_map, node_order_by_presence(src_map)


def scale_in_rank_order(g, values):
    """``values`` ([E] or [E, H] by edge id) in the order of the grouping ``g`` (whose second payload is the edge id), or None.
    For a scale that is the same tensor step after step (an edge norm): built at its SECOND sighting -- a scale that changes every
    step never pays for it -- and kept with the grouping, one per grouping (a new tensor replaces it); the entry holds the source
    tensor, so its address cannot come back with other contents, and (data_ptr, numel, _version) catches in-place edits."""
    if g is None or values is None:
        return None
    ident = _plan._ident(values)
    if ident[2] == _plan.NO_VERSION:  # (an inference tensor: an edit in place could not be seen -- the by-edge-id gather every time)
        return None
    with _derived_lock:
        hit = getattr(g, "_scale_sorted", None)
        if hit is not None and hit[0] == ident:
            return hit[2]
        if getattr(g, "_scale_seen", None) != ident:
            g._scale_seen, g._scale_sorted = ident, None
            return None
        with _plan.building():  # (kept with the grouping: a normal tensor whatever the caller's mode)
            out = torch.empty_like(values, memory_format=torch.contiguous_format)
        H = values.numel() // max(1, values.shape[0])
        _call(values, "het_grouping_gather_payload1", g.handle, _p(values), H, _p(out), _stream(values))
        g._scale_sorted = (ident, values, out)
        return out


def _rgcn_layer_forward(entry, plan, x, weights, norm, bias):
    """rgcn_layer_forward / _bf16 behind their tensor checks: ret has x's dtype, the kept sums are fp32."""
    gd, _, dst_map, dst_order, _, _ = plan
    R, K, D = weights.shape
    N = dst_map.shape[1]
    ssum = torch.empty((max(1, gd.num_segments), K), dtype=torch.float32, device=x.device)
    ret = torch.empty((N, D), dtype=x.dtype, device=x.device)
    _call(ret, entry, gd.handle, R, N, _p(x), _p(weights), _p(norm), _p(scale_in_rank_order(gd, norm)), _p(bias), _p(dst_map),
          _p(dst_order), _p(ssum), _p(ret), K, D, _stream(ret))
    return ret, ssum


def _rgcn_layer_backward(entry, plan, ssum, weights_t, norm, gradout, want_bias, want_x):
    """rgcn_layer_backward / _bf16 behind their tensor checks: grad_x has gradout's dtype, grad_w and grad_bias are fp32."""
    gd, gs, _, _, src_map, src_order = plan
    R, D, K = weights_t.shape
    N = src_map.shape[1]
    dev = gradout.device
    grad_x = torch.empty((N, K), dtype=gradout.dtype, device=dev) if want_x else None
    grad_w = torch.empty((R, K, D), dtype=torch.float32, device=dev)
    grad_bias = torch.empty((D,), dtype=torch.float32, device=dev) if want_bias else None
    ws, nbytes = _workspace(gradout, "het_rgcn_layer_backward_workspace", gs.num_segments, D)
    _call(gradout, entry, gs.handle, gd.handle, R, N, gradout.shape[0], _p(ssum), _p(weights_t), _p(norm),
          _p(scale_in_rank_order(gs, norm) if want_x else None), _p(gradout), _p(src_map), _p(src_order), _p(grad_x), _p(grad_w),
          _p(grad_bias), K, D, _p(ws), nbytes, _stream(gradout))
    return grad_x, grad_w, grad_bias


def rgcn_layer_forward(plan, x, weights, norm, bias):
    """(ret [N,D], ssum [S_col,K]) of het_rgcn_layer_forward: ret = bias + SUM_r (SUM_e norm x[src]) . W[r]."""
    _chk("rgcn_layer_forward", tuple(t for t in (x, weights, norm, bias) if t is not None))
    return _rgcn_layer_forward("het_rgcn_layer_forward", plan, x, weights, norm, bias)


def rgcn_layer_backward(plan, ssum, weights_t, norm, gradout, want_bias: bool, want_x: bool = True):
    """(grad_x [N,K] or None, grad_w [R,K,D], grad_bias [D] or None) of het_rgcn_layer_backward."""
    _chk("rgcn_layer_backward", (ssum, weights_t, norm, gradout))
    return _rgcn_layer_backward("het_rgcn_layer_backward", plan, ssum, weights_t, norm, gradout, want_bias, want_x)


def _chk_bf16(name: str, rows=(), floats=()):
    """The bf16 layer entries: activation rows (``rows``) contiguous bfloat16 GPU tensors, everything else as _chk."""
    for t in rows:
        if not (t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous()):
            raise _lib.HetError(f"{name}: expected contiguous bfloat16 GPU activation rows, got {t.dtype} on {t.device}"
                                f"{'' if t.is_contiguous() else ' (non-contiguous)'}")
    _chk(name, floats)


def rgcn_layer_forward_bf16(plan, x, weights, norm, bias):
    """rgcn_layer_forward with bf16 activations (het_rgcn_layer_forward_bf16): x and the returned ret [N,D] bf16; weights, norm,
    bias and the kept sums ssum [S_col,K] fp32."""
    _chk_bf16("rgcn_layer_forward_bf16", (x,), tuple(t for t in (weights, norm, bias) if t is not None))
    return _rgcn_layer_forward("het_rgcn_layer_forward_bf16", plan, x, weights, norm, bias)


def rgcn_layer_backward_bf16(plan, ssum, weights_t, norm, gradout, want_bias: bool, want_x: bool = True):
    """rgcn_layer_backward with bf16 activations (het_rgcn_layer_backward_bf16): gradout and grad_x [N,K] bf16; grad_w [R,K,D]
    and grad_bias [D] fp32."""
    _chk_bf16("rgcn_layer_backward_bf16", (gradout,), (ssum, weights_t, norm))
    return _rgcn_layer_backward("het_rgcn_layer_backward_bf16", plan, ssum, weights_t, norm, gradout, want_bias, want_x)


# ---- the RGCN layer with block-diagonal relation weights (include/het_amd.h: het_rgcn_bdd_layer_forward; csrc/rgcn_bdd.hip) ----
def rgcn_bdd_ok(R: int, K: int, D: int, B: int) -> bool:
    """Shapes of the native bdd layer (het_rgcn_bdd_layer_ok): K, D in {32, 64, 128}, K / B and D / B in {4, 8, 16, 32}, R >= 1."""
    return bool(_lib.lib().het_rgcn_bdd_layer_ok(int(R), int(K), int(D), int(B)))


def rgcn_bdd_params() -> Dict[str, int]:
    """The launch constants of csrc/rgcn_bdd.hip (het_rgcn_bdd_params; runs on the host): ``chunk_rows`` (relation, node) rows per
    weight-gradient work item, ``lds_weight_bytes`` up to which the blocks of all relations are held in LDS, ``block`` threads per
    workgroup, block sides from ``min_side`` to ``max_side``, ``colsum_blocks`` partial rows of the bias gradient."""
    L = _lib.lib()
    out = (C.c_int64 * 6)()
    rc = L.het_rgcn_bdd_params(out)
    if rc != 0:
        raise _lib.HetError(f"het_rgcn_bdd_params failed (code {rc}): {L.het_last_error().decode()}")
    return dict(zip(("chunk_rows", "lds_weight_bytes", "block", "min_side", "max_side", "colsum_blocks"), (int(v) for v in out)))


def rgcn_bdd_lds_relations(K: int, D: int, B: int) -> int:
    """The largest relation count whose blocks the node pass holds in LDS at this shape (one more reads them through the caches)."""
    return rgcn_bdd_params()["lds_weight_bytes"] // (4 * K * D // B)


def grouping_node_rows(g, rel_ptrs, keys, num_keys: int):
    """(node_ptr [num_keys + 1], ent_row [S], ent_rel [S]) int32 of het_grouping_node_rows: per node the segments of the grouping
    ``g`` of ``keys`` by (relation, key) that belong to it, in ascending relation order, and their relations.  Built once per graph
    on the device and cached by the identity of the lists the grouping was built from, like the segment maps."""
    def build():
        S = g.num_segments
        node_ptr = torch.empty(num_keys + 1, dtype=torch.int32, device=keys.device)
        ent_row = torch.empty(max(1, S), dtype=torch.int32, device=keys.device)
        ent_rel = torch.empty(max(1, S), dtype=torch.int32, device=keys.device)
        _call(keys, "het_grouping_node_rows", g.handle, num_keys, _p(node_ptr), _p(ent_row), _p(ent_rel), _stream(keys))
        return node_ptr, ent_row[:S], ent_rel[:S]
    return _derived_get(("noderows", num_keys), (rel_ptrs, keys), build)


def rgcn_bdd_layer_plan(rel_ptrs, eids, row, col, num_nodes: int):
    """What the native bdd layer needs per graph: (by_rel_dst, by_rel_src, dst_rows, src_rows) -- the groupings of the two-call layer
    and their per-node row lists (grouping_node_rows) --, or None without groupings."""
    gd = _plan.get_grouping(rel_ptrs, col, num_nodes, row, eids)
    gs = _plan.get_grouping(rel_ptrs, row, num_nodes, col, eids)
    if gd is None or gs is None:
        return None
    return gd, gs, grouping_node_rows(gd, rel_ptrs, col, num_nodes), grouping_node_rows(gs, rel_ptrs, row, num_nodes)


def rgcn_bdd_layer_forward(plan, x, weights, norm, bias):
    """(ret [N,D], ssum [S_col,K]) of het_rgcn_bdd_layer_forward; weights [R,B,K/B,D/B]."""
    _chk("rgcn_bdd_layer_forward", tuple(t for t in (x, weights, norm, bias) if t is not None))
    gd, _, (node_ptr, ent_row, ent_rel), _ = plan
    R, B, si, so = weights.shape
    K, D, N = B * si, B * so, node_ptr.numel() - 1
    ssum = torch.empty((max(1, gd.num_segments), K), dtype=torch.float32, device=x.device)
    ret = torch.empty((N, D), dtype=torch.float32, device=x.device)
    _call(ret, "het_rgcn_bdd_layer_forward", gd.handle, R, N, _p(x), _p(weights), _p(norm), _p(scale_in_rank_order(gd, norm)), _p(bias),
          _p(node_ptr), _p(ent_row), _p(ent_rel), _p(ssum), _p(ret), K, D, B, _stream(ret))
    return ret, ssum


def rgcn_bdd_layer_backward(plan, ssum, weights_t, norm, gradout, want_bias: bool, want_x: bool = True):
    """(grad_x [N,K] or None, grad_w [R,B,K/B,D/B], grad_bias [D] or None) of het_rgcn_bdd_layer_backward; weights_t [R,B,D/B,K/B]:
    every block transposed."""
    _chk("rgcn_bdd_layer_backward", (ssum, weights_t, norm, gradout))
    gd, gs, _, (node_ptr, ent_row, ent_rel) = plan
    R, B, so, si = weights_t.shape
    K, D, N = B * si, B * so, node_ptr.numel() - 1
    dev = gradout.device
    grad_x = torch.empty((N, K), dtype=torch.float32, device=dev) if want_x else None
    grad_w = torch.empty((R, B, si, so), dtype=torch.float32, device=dev)
    grad_bias = torch.empty((D,), dtype=torch.float32, device=dev) if want_bias else None
    ws, nbytes = _workspace(gradout, "het_rgcn_bdd_layer_backward_workspace", gs.num_segments, gd.num_segments, R, K, D, B)
    _call(gradout, "het_rgcn_bdd_layer_backward", gs.handle, gd.handle, R, N, gradout.shape[0], _p(ssum), _p(weights_t), _p(norm),
          _p(scale_in_rank_order(gs, norm) if want_x else None), _p(gradout), _p(node_ptr), _p(ent_row), _p(ent_rel), _p(grad_x),
          _p(grad_w), _p(grad_bias), K, D, B, _p(ws), nbytes, _stream(gradout))
    return grad_x, grad_w, grad_bias


# ---- the HGT layer with bf16 activations (backend/hgt_fused_layer.py): activation rows bf16, everything else fp32 ----
def rows_matmul_bf16_ok(K: int, X: int) -> bool:
    """Shapes het_rows_matmul_bf16 / het_rows_matmul_backward_dw_bf16 cover."""
    return K in (32, 64) and X in (32, 64, 128)


def rows_matmul_bf16(rel_ptrs, gather_idx, scatter_idx, weights, x, out):
    """out[scatter_idx[i]] = x[gather_idx[i]] . weights[r(i)] (include/het_amd.h: het_rows_matmul_bf16): x [*,K] and out [*,X] bf16,
    weights [R,1,K,X] fp32; a missing list means row i.  Plain stores: the output rows of the call are distinct."""
    lists = tuple(t for t in (gather_idx, scatter_idx) if t is not None)
    _chk_bf16("rows_matmul_bf16", (x, out), (weights,))
    _chk("rows_matmul_bf16", (), (rel_ptrs,) + lists)
    R, _, K, X = weights.shape
    n = lists[0].numel() if lists else x.shape[0]
    if x.shape[-1] != K or out.shape[-1] != X or (gather_idx is None and x.shape[0] < n) or (scatter_idx is None and out.shape[0] < n):
        raise _lib.HetError(f"rows_matmul_bf16: x {tuple(x.shape)} / out {tuple(out.shape)} do not fit weights {tuple(weights.shape)} and {n} rows")
    _call(out, "het_rows_matmul_bf16", _p(rel_ptrs), R, _p(gather_idx), _p(scatter_idx), n, _p(weights), _p(x), _p(out), K, X,
          _stream(out))


def rows_matmul_backward_dw_bf16(rel_ptrs, gather_idx, x, gradout, grad_w, accumulate: bool, g_rows=None):
    """grad_w[r(i)] (+)= x[gather_idx[i]]^T (x) gradout[g_rows[i]] (het_rows_matmul_backward_dw_bf16 / _bf16_bf16): x bf16, gradout fp32 or bf16,
    grad_w [R,1,K,X] fp32."""
    lists = tuple(t for t in (gather_idx, g_rows) if t is not None)
    g_bf16 = gradout.dtype == torch.bfloat16
    _chk_bf16("rows_matmul_backward_dw_bf16", (x, gradout) if g_bf16 else (x,), (grad_w,) if g_bf16 else (gradout, grad_w))
    _chk("rows_matmul_backward_dw_bf16", (), (rel_ptrs,) + lists)
    R, _, K, X = grad_w.shape
    n = lists[0].numel() if lists else gradout.shape[0]
    if x.shape[-1] != K or gradout.shape[-1] != X or (gather_idx is None and x.shape[0] < n) or (g_rows is None and gradout.shape[0] < n):
        raise _lib.HetError(f"rows_matmul_backward_dw_bf16: x {tuple(x.shape)} / gradout {tuple(gradout.shape)} do not fit grad_w "
                            f"{tuple(grad_w.shape)} and {n} rows")
    _call(gradout, "het_rows_matmul_backward_dw_bf16_bf16" if g_bf16 else "het_rows_matmul_backward_dw_bf16", _p(rel_ptrs), R,
          _p(gather_idx), _p(g_rows), n, _p(x), _p(gradout), _p(grad_w), K, X, int(accumulate), _stream(gradout))


def node_rows_matmul_sum_bf16(n_begin, n_end, sources, out, node_order=None):
    """node_rows_matmul_sum with bf16 output rows (het_node_rows_matmul_sum_bf16): the source rows and weights are fp32."""
    _chk_bf16("node_rows_matmul_sum_bf16", (out,), tuple(t for src in sources for t in (src[0], src[3])))
    _node_rows_matmul_sum("het_node_rows_matmul_sum_bf16", n_begin, n_end, sources, out, node_order, False)


def _hgt_bf16_shapes(name, kv_c, q, lsum, out):
    N, H = lsum.shape
    D = out.numel() // max(1, N * H)
    if q.numel() != N * H * D or out.numel() != N * H * D or kv_c.numel() != kv_c.shape[0] * 2 * H * D:
        raise _lib.HetError(f"{name}: kv_c {tuple(kv_c.shape)}, q {tuple(q.shape)}, out {tuple(out.shape)} do not fit lsum {tuple(lsum.shape)}")


def hgt_aggregate_compact_bf16(groupings, kv_c, q, lsum, out, workspace=None):
    """hgt_aggregate_compact with bf16 rows (het_hgt_aggregate_compact_bf16): kv_c, q and out bf16, lsum fp32.  ``workspace``: a
    float32 tensor of the caller instead of the one allocated here (the C entry checks its size and alignment)."""
    _chk_bf16("hgt_aggregate_compact_bf16", (kv_c, q, out), (lsum,))
    _hgt_bf16_shapes("hgt_aggregate_compact_bf16", kv_c, q, lsum, out)
    _hgt_aggregate_compact("het_hgt_aggregate_compact_bf16", groupings, kv_c, q, lsum, out, workspace)


def hgt_backward_compact_bf16(groupings, kv_c, q, lsum, out, gradout, grad_kv_c, grad_q, workspace=None):
    """hgt_backward_compact with bf16 rows (het_hgt_backward_compact_bf16): kv_c, q, out and gradout bf16; lsum, grad_kv_c and
    grad_q fp32."""
    _chk_bf16("hgt_backward_compact_bf16", (kv_c, q, out, gradout), (lsum, grad_kv_c, grad_q))
    _hgt_bf16_shapes("hgt_backward_compact_bf16", kv_c, q, lsum, out)
    if gradout.numel() != out.numel() or grad_q.numel() != q.numel() or grad_kv_c.numel() != kv_c.numel():
        raise _lib.HetError("hgt_backward_compact_bf16: gradient shapes do not match their tensors")
    _hgt_backward_compact("het_hgt_backward_compact_bf16", groupings, kv_c, q, lsum, out, gradout, grad_kv_c, grad_q, workspace)


def _rgcn_maps(d: Dict[str, Tensor], direct: bool):
    if direct:
        return d["inverse_indices_row"], None
    return d["rel_ptrs_row"], d["node_indices_row"]


@_op("rgcn_node_mean_aggregation_compact_as_of_node_separate_coo(Tensor separate_coo_eids, Tensor separate_coo_rel_ptrs, "
     "Tensor separate_coo_row_indices, Tensor separate_coo_col_indices, Dict(str, Tensor) args_tensor_dict, "
     "Tensor feat_src, Tensor enorm, Tensor(a!) ret, bool DirectIndexFlag) -> ()")
def rgcn_node_mean_aggregation_compact_as_of_node_separate_coo(separate_coo_eids, separate_coo_rel_ptrs,
                                                               separate_coo_row_indices, separate_coo_col_indices,
                                                               args_tensor_dict, feat_src, enorm, ret, DirectIndexFlag):
    a, b = _rgcn_maps(args_tensor_dict, DirectIndexFlag)
    _chk("rgcn_node_mean_aggregation_compact_as_of_node_separate_coo", (feat_src, enorm, ret),
         (separate_coo_eids, separate_coo_rel_ptrs, separate_coo_row_indices, separate_coo_col_indices, a)
         + ((b,) if b is not None else ()))
    N = ret.shape[0]
    g = None
    if _plan.is_enabled() and separate_coo_eids.numel() > 0:
        crow = _src_rows_by_position(4 if DirectIndexFlag else 3, (a, b, None, None), separate_coo_rel_ptrs,
                                     separate_coo_row_indices, separate_coo_eids)
        g = _plan.get_grouping(None, separate_coo_col_indices, N, crow, separate_coo_eids)
    _call(ret, "het_rgcn_node_mean_aggregation_compact_as_of_node_separate_coo", _p(separate_coo_eids),
          _p(separate_coo_rel_ptrs), _p(separate_coo_row_indices), _p(separate_coo_col_indices),
          separate_coo_rel_ptrs.numel() - 1, separate_coo_eids.numel(), N, _p(a), _p(b), _p(feat_src), _p(enorm), _p(ret),
          ret.numel() // max(1, N), int(DirectIndexFlag), None if g is None else g.handle, _stream(ret))


@_op("backward_rgcn_node_mean_aggregation_compact_as_of_node_separate_coo(Tensor separate_coo_eids, "
     "Tensor separate_coo_rel_ptrs, Tensor separate_coo_row_indices, Tensor separate_coo_col_indices, "
     "Dict(str, Tensor) args_tensor_dict, Tensor feat_src, Tensor enorm, Tensor ret, Tensor gradout, "
     "Tensor(a!) grad_feat_src, bool DirectIndexFlag) -> ()")
def backward_rgcn_node_mean_aggregation_compact_as_of_node_separate_coo(separate_coo_eids, separate_coo_rel_ptrs,
                                                                        separate_coo_row_indices,
                                                                        separate_coo_col_indices, args_tensor_dict,
                                                                        feat_src, enorm, ret, gradout, grad_feat_src,
                                                                        DirectIndexFlag):
    a, b = _rgcn_maps(args_tensor_dict, DirectIndexFlag)
    _chk("backward_rgcn_node_mean_aggregation_compact_as_of_node_separate_coo", (feat_src, enorm, ret, gradout, grad_feat_src),
         (separate_coo_eids, separate_coo_rel_ptrs, separate_coo_row_indices, separate_coo_col_indices, a)
         + ((b,) if b is not None else ()))
    N = ret.shape[0]
    g = None
    if _plan.is_enabled() and separate_coo_eids.numel() > 0:
        crow = _src_rows_by_position(4 if DirectIndexFlag else 3, (a, b, None, None), separate_coo_rel_ptrs,
                                     separate_coo_row_indices, separate_coo_eids)
        g = _plan.get_grouping(None, crow, grad_feat_src.shape[0], separate_coo_col_indices, separate_coo_eids)
    _call(ret, "het_backward_rgcn_node_mean_aggregation_compact_as_of_node_separate_coo", _p(separate_coo_eids),
          _p(separate_coo_rel_ptrs), _p(separate_coo_row_indices), _p(separate_coo_col_indices),
          separate_coo_rel_ptrs.numel() - 1, separate_coo_eids.numel(), N, _p(a), _p(b), _p(feat_src), _p(enorm), _p(ret),
          _p(gradout), _p(grad_feat_src), ret.numel() // max(1, N), int(DirectIndexFlag),
          None if g is None else g.handle, grad_feat_src.shape[0], _stream(ret))


K = getattr(torch.ops, NAMESPACE)
REGISTERED_OPS = tuple(_registered)


# ------------------------------------------------------------------------------------
# HGT
# ------------------------------------------------------------------------------------
def _ip_maps(d: Dict[str, Tensor], kind: int):
    if kind == 0:
        return None, None
    if kind == 1:
        return d["unique_srcs_and_dests_rel_ptrs"], d["unique_srcs_and_dests_node_indices"]
    if kind == 2:
        return d["edata_idx_to_inverse_idx"], None
    raise _lib.HetError(f"rgnn_inner_product_right_node: CompactAsOfNodeKind {kind} not supported")


def _ip_direct(d: Dict[str, Tensor], kind: int, rel_ptrs, col, eids):
    """(kind, map_a, map_b) as handed to the C entry points: the binary-search kind 1 is turned into the direct-index
    kind 2 once per graph (left row of every edge id; cached), which is what the fast row kernels read."""
    a, b = _ip_maps(d, kind)
    if kind != 1 or not _plan.is_enabled() or eids.numel() == 0:
        return kind, a, b
    def build():
        lrow = _rows_by_search(rel_ptrs, col, a, b)
        m = torch.empty(int(eids.max().item()) + 1, dtype=torch.int64, device=col.device)
        m[eids] = lrow
        return m

    hit = (_derived_get("ipmap", (a, b, rel_ptrs, col, eids), build),)
    return 2, hit[0], None


@_op("rgnn_inner_product_right_node_separatecoo(Dict(str, Tensor) arg_tensor_dict, int IntKind, "
     "Tensor separate_coo_rel_ptrs, Tensor separate_coo_eids, Tensor separate_coo_row_indices, "
     "Tensor separate_coo_col_indices, Tensor left_side_data, Tensor right_node_vectors, "
     "Tensor(a!) edge_inner_product) -> ()")
def rgnn_inner_product_right_node_separatecoo(arg_tensor_dict, IntKind, separate_coo_rel_ptrs, separate_coo_eids,
                                              separate_coo_row_indices, separate_coo_col_indices, left_side_data,
                                              right_node_vectors, edge_inner_product):
    a, b = _ip_maps(arg_tensor_dict, IntKind)
    _chk("rgnn_inner_product_right_node_separatecoo", (left_side_data, right_node_vectors, edge_inner_product),
         (separate_coo_rel_ptrs, separate_coo_eids, separate_coo_row_indices, separate_coo_col_indices)
         + tuple(t for t in (a, b) if t is not None))
    IntKind, a, b = _ip_direct(arg_tensor_dict, IntKind, separate_coo_rel_ptrs, separate_coo_col_indices, separate_coo_eids)
    H = edge_inner_product.shape[1]
    D = right_node_vectors.numel() // max(1, right_node_vectors.shape[0] * H)
    _call(edge_inner_product, "het_rgnn_inner_product_right_node_separatecoo", IntKind, _p(a), _p(b),
          _p(separate_coo_rel_ptrs), _p(separate_coo_eids), _p(separate_coo_row_indices), _p(separate_coo_col_indices),
          separate_coo_rel_ptrs.numel() - 1, separate_coo_eids.numel(), _p(left_side_data), _p(right_node_vectors),
          _p(edge_inner_product), H, D, _stream(edge_inner_product))


@_op("backward_inner_product_right_node_separatecoo(Dict(str, Tensor) arg_tensor_dict, int IntKind, "
     "Tensor separate_coo_rel_ptrs, Tensor separate_coo_eids, Tensor separate_coo_row_indices, "
     "Tensor separate_coo_col_indices, Tensor left_side_data, Tensor right_node_vectors, Tensor gradout, "
     "Tensor(a!) grad_left_side_data, Tensor(b!) grad_right_node_vectors) -> ()")
def backward_inner_product_right_node_separatecoo(arg_tensor_dict, IntKind, separate_coo_rel_ptrs, separate_coo_eids,
                                                  separate_coo_row_indices, separate_coo_col_indices, left_side_data,
                                                  right_node_vectors, gradout, grad_left_side_data,
                                                  grad_right_node_vectors):
    a, b = _ip_maps(arg_tensor_dict, IntKind)
    _chk("backward_inner_product_right_node_separatecoo",
         (left_side_data, right_node_vectors, gradout, grad_left_side_data, grad_right_node_vectors),
         (separate_coo_rel_ptrs, separate_coo_eids, separate_coo_row_indices, separate_coo_col_indices)
         + tuple(t for t in (a, b) if t is not None))
    inner_product_backward(arg_tensor_dict, IntKind, separate_coo_rel_ptrs, separate_coo_eids, separate_coo_row_indices,
                           separate_coo_col_indices, left_side_data, right_node_vectors, gradout, grad_left_side_data,
                           grad_right_node_vectors, accumulate=True, checked=True)


def inner_product_backward(arg_tensor_dict, IntKind, separate_coo_rel_ptrs, separate_coo_eids, separate_coo_row_indices,
                           separate_coo_col_indices, left_side_data, right_node_vectors, gradout, grad_left_side_data,
                           grad_right_node_vectors, accumulate: bool, checked: bool = False):
    a, b = _ip_maps(arg_tensor_dict, IntKind)
    if not checked:
        _chk("backward_inner_product_right_node_separatecoo",
             (left_side_data, right_node_vectors, gradout, grad_left_side_data, grad_right_node_vectors),
             (separate_coo_rel_ptrs, separate_coo_eids, separate_coo_row_indices, separate_coo_col_indices)
             + tuple(t for t in (a, b) if t is not None))
    H = gradout.shape[1]
    D = right_node_vectors.numel() // max(1, right_node_vectors.shape[0] * H)
    IntKind, a, b = _ip_direct(arg_tensor_dict, IntKind, separate_coo_rel_ptrs, separate_coo_col_indices, separate_coo_eids)
    g = gl = None
    if IntKind in (0, 2) and _plan.is_enabled():
        if IntKind == 0:
            lrow = separate_coo_eids
        else:
            lrow = _derived_get("iplrow", (a, separate_coo_eids), lambda: a[separate_coo_eids].contiguous())
            # compact left rows are shared by many edges: their gradient is a segmented sum over the edges of a row
            gl = _plan.get_grouping(None, lrow, left_side_data.shape[0], separate_coo_row_indices, separate_coo_eids)
        g = _plan.get_grouping(None, separate_coo_row_indices, right_node_vectors.shape[0], lrow, separate_coo_eids)
    _call(gradout, "het_backward_inner_product_right_node_separatecoo", IntKind, _p(a), _p(b),
          _p(separate_coo_rel_ptrs), _p(separate_coo_eids), _p(separate_coo_row_indices), _p(separate_coo_col_indices),
          separate_coo_rel_ptrs.numel() - 1, separate_coo_eids.numel(), _p(left_side_data), _p(right_node_vectors),
          _p(gradout), _p(grad_left_side_data), _p(grad_right_node_vectors), H, D, int(accumulate),
          None if g is None else g.handle, None if gl is None else gl.handle, left_side_data.shape[0],
          right_node_vectors.shape[0], _stream(gradout))


@_op("hgt_full_graph_edge_softmax_ops_separate_coo(Tensor row_indices, Tensor col_indices, Tensor eids, Tensor rel_ptrs, "
     "Tensor unnormalized_attn_score, Tensor mu, Tensor(a!) edgesoftmax_sum_per_node, "
     "Tensor(b!) mu_softmax_applied_unnormalized_attn_score, Tensor(c!) normalized_attn_score) -> ()")
def hgt_full_graph_edge_softmax_ops_separate_coo(row_indices, col_indices, eids, rel_ptrs, unnormalized_attn_score, mu,
                                                 edgesoftmax_sum_per_node, mu_softmax_applied_unnormalized_attn_score,
                                                 normalized_attn_score):
    _chk("hgt_full_graph_edge_softmax_ops_separate_coo",
         (unnormalized_attn_score, mu, edgesoftmax_sum_per_node, mu_softmax_applied_unnormalized_attn_score,
          normalized_attn_score), (row_indices, col_indices, eids, rel_ptrs))
    H = mu.shape[1]
    N = edgesoftmax_sum_per_node.shape[0]
    g = _by_dst(0, None, rel_ptrs, row_indices, col_indices, eids, N) if H % 4 == 0 and eids.numel() > 0 else None
    _call(mu, "het_hgt_full_graph_edge_softmax_ops_separate_coo", _p(row_indices), _p(col_indices), _p(eids),
          _p(rel_ptrs), rel_ptrs.numel() - 1, eids.numel(), N,
          _p(unnormalized_attn_score), _p(mu), _p(edgesoftmax_sum_per_node),
          _p(mu_softmax_applied_unnormalized_attn_score), _p(normalized_attn_score), H,
          None if g is None else g.handle, _stream(mu))


@_op("backward_hgt_full_graph_enorm_to_unnormalized_attn_score_separate_coo(Tensor row_indices, Tensor col_indices, "
     "Tensor eids, Tensor rel_ptrs, Tensor unnormalized_attn_score, Tensor normalized_attn_score, "
     "Tensor grad_normalized_attn_score, Tensor mu, Tensor(a!) grad_unnormalized_attn_score, Tensor(b!) grad_mu, "
     "Tensor(c!) sum_incoming_edges_product_softmax_score) -> ()")
def backward_hgt_full_graph_enorm_to_unnormalized_attn_score_separate_coo(
        row_indices, col_indices, eids, rel_ptrs, unnormalized_attn_score, normalized_attn_score,
        grad_normalized_attn_score, mu, grad_unnormalized_attn_score, grad_mu, sum_incoming_edges_product_softmax_score):
    _chk("backward_hgt_full_graph_enorm_to_unnormalized_attn_score_separate_coo",
         (unnormalized_attn_score, normalized_attn_score, grad_normalized_attn_score, mu, grad_unnormalized_attn_score,
          grad_mu, sum_incoming_edges_product_softmax_score), (row_indices, col_indices, eids, rel_ptrs))
    H = mu.shape[1]
    N = sum_incoming_edges_product_softmax_score.shape[0]
    g = _by_dst(0, None, rel_ptrs, row_indices, col_indices, eids, N) if H % 4 == 0 and eids.numel() > 0 else None
    _call(mu, "het_backward_hgt_full_graph_enorm_to_unnormalized_attn_score_separate_coo", _p(row_indices),
          _p(col_indices), _p(eids), _p(rel_ptrs), rel_ptrs.numel() - 1, eids.numel(),
          N, _p(unnormalized_attn_score), _p(normalized_attn_score),
          _p(grad_normalized_attn_score), _p(mu), _p(grad_unnormalized_attn_score), _p(grad_mu),
          _p(sum_incoming_edges_product_softmax_score), H, None if g is None else g.handle, _stream(mu))


# HGT's unfused aggregation on the CSR layouts (HGTOps.inc.h IntegratedCSR; include/het_amd.h a10c).  The fast paths take the
# positions grouped by destination: an in-CSR's expanded rows, an out-CSR's col_indices (payload0 = eids, payload1 = reltypes).
def _csr_by_dst(dst, num_nodes, eids, reltypes):
    return _plan.get_grouping(None, dst, num_nodes, eids, reltypes) if eids.numel() > 0 else None


def _incsr_by_dst(row_ptr, eids, reltypes):
    if eids.numel() == 0 or not _plan.is_enabled():
        return None
    dst, _ = _csr_expanded_rows(row_ptr, eids.numel())
    return _csr_by_dst(dst, row_ptr.numel() - 1, eids, reltypes)


@_op("hgt_full_graph_edge_softmax_ops_csr(Tensor row_ptr, Tensor col_indices, Tensor eids, Tensor reltypes, "
     "Tensor unnormalized_attn_score, Tensor mu, Tensor(a!) edgesoftmax_sum_per_node, "
     "Tensor(b!) mu_softmax_applied_unnormalized_attn_score, Tensor(c!) normalized_attn_score) -> ()")
def hgt_full_graph_edge_softmax_ops_csr(row_ptr, col_indices, eids, reltypes, unnormalized_attn_score, mu,
                                        edgesoftmax_sum_per_node, mu_softmax_applied_unnormalized_attn_score,
                                        normalized_attn_score):
    _chk("hgt_full_graph_edge_softmax_ops_csr",
         (unnormalized_attn_score, mu, edgesoftmax_sum_per_node, mu_softmax_applied_unnormalized_attn_score,
          normalized_attn_score), (row_ptr, col_indices, eids, reltypes))
    H, N = mu.shape[1], edgesoftmax_sum_per_node.shape[0]
    g = _incsr_by_dst(row_ptr, eids, reltypes) if H % 4 == 0 else None
    _call(mu, "het_hgt_full_graph_edge_softmax_ops_csr", _p(row_ptr), row_ptr.numel(), _p(col_indices), _p(eids),
          _p(reltypes), N, eids.numel(), _p(unnormalized_attn_score), _p(mu), _p(edgesoftmax_sum_per_node),
          _p(mu_softmax_applied_unnormalized_attn_score), _p(normalized_attn_score), H, None if g is None else g.handle,
          _stream(mu))


@_op("hgt_full_graph_message_mean_aggregation_csr(Tensor incsr_row_ptrs, Tensor incsr_col_indices, Tensor incsr_reltypes, "
     "Tensor incsr_eids, Tensor edge_messages, Tensor edge_attn_score, Tensor edgesoftmax_sum_per_node, Tensor mu, "
     "Tensor(a!) ret) -> ()")
def hgt_full_graph_message_mean_aggregation_csr(incsr_row_ptrs, incsr_col_indices, incsr_reltypes, incsr_eids, edge_messages,
                                                edge_attn_score, edgesoftmax_sum_per_node, mu, ret):
    _chk("hgt_full_graph_message_mean_aggregation_csr", (edge_messages, edge_attn_score, edgesoftmax_sum_per_node, mu, ret),
         (incsr_row_ptrs, incsr_col_indices, incsr_reltypes, incsr_eids))
    H, dk = edge_attn_score.shape[-1], edge_messages.shape[-1]
    g = _incsr_by_dst(incsr_row_ptrs, incsr_eids, incsr_reltypes)
    _call(ret, "het_hgt_full_graph_message_mean_aggregation_csr", _p(incsr_row_ptrs), incsr_row_ptrs.numel(),
          _p(incsr_col_indices), _p(incsr_reltypes), _p(incsr_eids), ret.shape[0], incsr_eids.numel(), _p(edge_messages),
          _p(edge_attn_score), _p(edgesoftmax_sum_per_node), _p(mu), _p(ret), H, dk, None if g is None else g.handle,
          _stream(ret))


@_op("backward_hgt_full_graph_message_mean_aggregation_csr(Tensor outcsr_row_ptrs, Tensor outcsr_col_indices, "
     "Tensor outcsr_reltypes, Tensor outcsr_eids, Tensor edgesoftmax_sum_per_node, Tensor normalized_attn_score, "
     "Tensor gradout, Tensor(a!) grad_message) -> ()")
def backward_hgt_full_graph_message_mean_aggregation_csr(outcsr_row_ptrs, outcsr_col_indices, outcsr_reltypes, outcsr_eids,
                                                         edgesoftmax_sum_per_node, normalized_attn_score, gradout,
                                                         grad_message):
    _chk("backward_hgt_full_graph_message_mean_aggregation_csr",
         (edgesoftmax_sum_per_node, normalized_attn_score, gradout, grad_message),
         (outcsr_row_ptrs, outcsr_col_indices, outcsr_reltypes, outcsr_eids))
    H, dk = normalized_attn_score.shape[-1], grad_message.shape[-1]
    _call(grad_message, "het_backward_hgt_full_graph_message_mean_aggregation_csr", _p(outcsr_row_ptrs),
          outcsr_row_ptrs.numel(), _p(outcsr_col_indices), _p(outcsr_reltypes), _p(outcsr_eids), gradout.shape[0],
          outcsr_eids.numel(), _p(edgesoftmax_sum_per_node), _p(normalized_attn_score), _p(gradout), _p(grad_message), H, dk,
          _stream(grad_message))


@_op("backward_hgt_full_graph_edge_softmax_ops_csr(Tensor outcsr_row_ptr, Tensor outcsr_col_indices, Tensor outcsr_eids, "
     "Tensor outcsr_reltypes, Tensor message, Tensor unnormalized_attn_score, Tensor normalized_attn_score, Tensor out, "
     "Tensor gradout, Tensor mu, Tensor(a!) grad_attn_score, Tensor(b!) grad_mu) -> ()")
def backward_hgt_full_graph_edge_softmax_ops_csr(outcsr_row_ptr, outcsr_col_indices, outcsr_eids, outcsr_reltypes, message,
                                                 unnormalized_attn_score, normalized_attn_score, out, gradout, mu,
                                                 grad_attn_score, grad_mu):
    _chk("backward_hgt_full_graph_edge_softmax_ops_csr",
         (message, unnormalized_attn_score, normalized_attn_score, out, gradout, mu, grad_attn_score, grad_mu),
         (outcsr_row_ptr, outcsr_col_indices, outcsr_eids, outcsr_reltypes))
    H, dk, N = grad_attn_score.shape[-1], message.shape[-1], gradout.shape[0]
    # destination-major view of the out-CSR: its positions grouped by col_indices (cached per graph)
    g = _csr_by_dst(outcsr_col_indices, N, outcsr_eids, outcsr_reltypes)
    _call(grad_attn_score, "het_backward_hgt_full_graph_edge_softmax_ops_csr", _p(outcsr_row_ptr), outcsr_row_ptr.numel(),
          _p(outcsr_col_indices), _p(outcsr_eids), _p(outcsr_reltypes), N, outcsr_eids.numel(), mu.shape[0], _p(message),
          _p(unnormalized_attn_score), _p(normalized_attn_score), _p(out), _p(gradout), _p(mu), _p(grad_attn_score),
          _p(grad_mu), H, dk, None if g is None else g.handle, _stream(grad_attn_score))


@_op("backward_hgt_full_graph_enorm_to_unnormalized_attn_score_csr(Tensor incsr_row_ptr, Tensor incsr_col_indices, "
     "Tensor incsr_eids, Tensor incsr_reltypes, Tensor unnormalized_attn_score, Tensor normalized_attn_score, "
     "Tensor grad_normalized_attn_score, Tensor mu, Tensor(a!) grad_unnormalized_attn_score, Tensor(b!) grad_mu) -> ()")
def backward_hgt_full_graph_enorm_to_unnormalized_attn_score_csr(incsr_row_ptr, incsr_col_indices, incsr_eids, incsr_reltypes,
                                                                 unnormalized_attn_score, normalized_attn_score,
                                                                 grad_normalized_attn_score, mu, grad_unnormalized_attn_score,
                                                                 grad_mu):
    _chk("backward_hgt_full_graph_enorm_to_unnormalized_attn_score_csr",
         (unnormalized_attn_score, normalized_attn_score, grad_normalized_attn_score, mu, grad_unnormalized_attn_score,
          grad_mu), (incsr_row_ptr, incsr_col_indices, incsr_eids, incsr_reltypes))
    H, N = mu.shape[1], incsr_row_ptr.numel() - 1
    g = _incsr_by_dst(incsr_row_ptr, incsr_eids, incsr_reltypes) if H % 4 == 0 else None
    ws = None if g is None else torch.empty(max(1, N * H), dtype=torch.float32, device=mu.device)  # (split hub destinations)
    _call(mu, "het_backward_hgt_full_graph_enorm_to_unnormalized_attn_score_csr", _p(incsr_row_ptr), incsr_row_ptr.numel(),
          _p(incsr_col_indices), _p(incsr_eids), _p(incsr_reltypes), N, incsr_eids.numel(), mu.shape[0],
          _p(unnormalized_attn_score), _p(normalized_attn_score), _p(grad_normalized_attn_score), _p(mu),
          _p(grad_unnormalized_attn_score), _p(grad_mu), H, None if g is None else g.handle, _p(ws),
          0 if ws is None else ws.numel() * 4, _stream(mu))


@_op("hgt_full_graph_fused_message_calc_and_mean_aggregation_separate_coo(Tensor separate_coo_relptrs, "
     "Tensor separate_coo_eids, Tensor separate_coo_row_indices, Tensor separate_coo_col_indices, Tensor inputs, "
     "Tensor weights, Tensor edge_norm, Tensor(a!) new_h) -> ()")
def hgt_full_graph_fused_message_calc_and_mean_aggregation_separate_coo(separate_coo_relptrs, separate_coo_eids,
                                                                        separate_coo_row_indices,
                                                                        separate_coo_col_indices, inputs, weights,
                                                                        edge_norm, new_h):
    _chk("hgt_full_graph_fused_message_calc_and_mean_aggregation_separate_coo", (inputs, weights, edge_norm, new_h),
         (separate_coo_relptrs, separate_coo_eids, separate_coo_row_indices, separate_coo_col_indices))
    R, H, dk, dout = weights.shape
    g = _plan.get_grouping(separate_coo_relptrs, separate_coo_col_indices, new_h.shape[0], separate_coo_row_indices,
                           separate_coo_eids)
    ws = None if g is None else torch.empty(max(1, g.num_segments) * H * dk, dtype=torch.float32, device=new_h.device)
    _call(new_h, "het_hgt_full_graph_fused_message_calc_and_mean_aggregation_separate_coo", _p(separate_coo_relptrs),
          _p(separate_coo_eids), _p(separate_coo_row_indices), _p(separate_coo_col_indices), R,
          separate_coo_eids.numel(), new_h.shape[0], _p(inputs), _p(weights), _p(edge_norm), _p(new_h), H, dk, dout,
          None if g is None else g.handle, _p(ws), 0 if ws is None else ws.numel() * 4, _stream(new_h))


@_op("backward_hgt_full_graph_fused_message_calc_and_mean_aggregation_separate_coo(Tensor separate_coo_relptrs, "
     "Tensor separate_coo_eids, Tensor separate_coo_row_indices, Tensor separate_coo_col_indices, Tensor inputs, "
     "Tensor weights_transposed, Tensor edge_norm, Tensor new_h, Tensor(a!) grad_input, Tensor(b!) grad_weights, "
     "Tensor(c!) grad_edge_norm, Tensor gradout) -> ()")
def backward_hgt_full_graph_fused_message_calc_and_mean_aggregation_separate_coo(
        separate_coo_relptrs, separate_coo_eids, separate_coo_row_indices, separate_coo_col_indices, inputs,
        weights_transposed, edge_norm, new_h, grad_input, grad_weights, grad_edge_norm, gradout):
    _chk("backward_hgt_full_graph_fused_message_calc_and_mean_aggregation_separate_coo",
         (inputs, weights_transposed, edge_norm, new_h, grad_input, grad_weights, grad_edge_norm, gradout),
         (separate_coo_relptrs, separate_coo_eids, separate_coo_row_indices, separate_coo_col_indices))
    R, H, dout, dk = weights_transposed.shape
    g = _plan.get_grouping(separate_coo_relptrs, separate_coo_row_indices, inputs.shape[0], separate_coo_col_indices,
                           separate_coo_eids)
    # segment sums of the gradient; for wide heads also the per-(relation, source) message rows and the untransposed weight
    ws = None if g is None else torch.empty(2 * max(1, g.num_segments) * H * dout + weights_transposed.numel(),
                                            dtype=torch.float32, device=gradout.device)
    _call(gradout, "het_backward_hgt_full_graph_fused_message_calc_and_mean_aggregation_separate_coo",
          _p(separate_coo_relptrs), _p(separate_coo_eids), _p(separate_coo_row_indices), _p(separate_coo_col_indices),
          R, separate_coo_eids.numel(), new_h.shape[0], _p(inputs), _p(weights_transposed), _p(edge_norm), _p(new_h),
          _p(grad_input), _p(grad_weights), _p(grad_edge_norm), _p(gradout), H, dk, dout,
          None if g is None else g.handle, _p(ws), 0 if ws is None else ws.numel() * 4, _stream(gradout))


@_op("hgt_full_graph_hetero_attention_ops_coo(Tensor separate_coo_row_indices, Tensor separate_coo_col_indices, "
     "Tensor separate_coo_eids, Tensor separate_coo_relptrs, Tensor applied_klinear_node_features, "
     "Tensor applied_qlinear_node_features, Tensor attn_score_weight, Tensor(a!) attn_score_inner_product, "
     "Tensor(b!) unnormalized_attn_score) -> ()")
def hgt_full_graph_hetero_attention_ops_coo(separate_coo_row_indices, separate_coo_col_indices, separate_coo_eids,
                                            separate_coo_relptrs, applied_klinear_node_features,
                                            applied_qlinear_node_features, attn_score_weight, attn_score_inner_product,
                                            unnormalized_attn_score):
    _chk("hgt_full_graph_hetero_attention_ops_coo",
         (applied_klinear_node_features, applied_qlinear_node_features, attn_score_weight, attn_score_inner_product,
          unnormalized_attn_score),
         (separate_coo_row_indices, separate_coo_col_indices, separate_coo_eids, separate_coo_relptrs))
    R, H, dk, dout = attn_score_weight.shape
    _call(unnormalized_attn_score, "het_hgt_full_graph_hetero_attention_ops_coo", _p(separate_coo_row_indices),
          _p(separate_coo_col_indices), _p(separate_coo_eids), _p(separate_coo_relptrs), R, separate_coo_eids.numel(),
          _p(applied_klinear_node_features), _p(applied_qlinear_node_features), _p(attn_score_weight),
          _p(attn_score_inner_product), _p(unnormalized_attn_score), H, dk, dout, _stream(unnormalized_attn_score))


@_op("backward_hgt_full_graph_hetero_attention_ops_coo(Tensor incsr_row_ptrs, Tensor incsr_col_indices, "
     "Tensor incsr_eids, Tensor incsr_reltypes, Tensor separate_coo_row_indices, Tensor separate_coo_col_indices, "
     "Tensor separate_coo_eids, Tensor separate_coo_relptrs, Tensor(a!) grad_attn_weight, "
     "Tensor attn_score_weight_transposed, Tensor applied_klinear_node_features, "
     "Tensor applied_qlinear_node_features, Tensor attn_score_inner_product, Tensor grad_unnorm_attn_score, "
     "Tensor(b!) grad_k, Tensor(c!) grad_q) -> ()")
def backward_hgt_full_graph_hetero_attention_ops_coo(incsr_row_ptrs, incsr_col_indices, incsr_eids, incsr_reltypes,
                                                     separate_coo_row_indices, separate_coo_col_indices,
                                                     separate_coo_eids, separate_coo_relptrs, grad_attn_weight,
                                                     attn_score_weight_transposed, applied_klinear_node_features,
                                                     applied_qlinear_node_features, attn_score_inner_product,
                                                     grad_unnorm_attn_score, grad_k, grad_q):
    _chk("backward_hgt_full_graph_hetero_attention_ops_coo",
         (grad_attn_weight, attn_score_weight_transposed, applied_klinear_node_features, applied_qlinear_node_features,
          attn_score_inner_product, grad_unnorm_attn_score, grad_k, grad_q),
         (separate_coo_row_indices, separate_coo_col_indices, separate_coo_eids, separate_coo_relptrs))
    R, H, dout, dk = attn_score_weight_transposed.shape
    nq = applied_qlinear_node_features.shape[0]
    gd = _plan.get_grouping(None, separate_coo_col_indices, nq, separate_coo_eids, None)
    gs = _plan.get_grouping(separate_coo_relptrs, separate_coo_row_indices, applied_klinear_node_features.shape[0],
                            separate_coo_col_indices, separate_coo_eids)
    ws = None if gs is None else torch.empty(max(1, gs.num_segments) * H * dout, dtype=torch.float32, device=grad_k.device)
    _call(grad_k, "het_backward_hgt_full_graph_hetero_attention_ops_coo", _p(separate_coo_row_indices),
          _p(separate_coo_col_indices), _p(separate_coo_eids), _p(separate_coo_relptrs), R, separate_coo_eids.numel(),
          _p(grad_attn_weight), _p(attn_score_weight_transposed), _p(applied_klinear_node_features),
          _p(applied_qlinear_node_features), _p(attn_score_inner_product), _p(grad_unnorm_attn_score), _p(grad_k),
          _p(grad_q), H, dk, dout, None if gd is None else gd.handle, None if gs is None else gs.handle, nq, _p(ws),
          0 if ws is None else ws.numel() * 4, _stream(grad_k))


REGISTERED_OPS = tuple(_registered)
