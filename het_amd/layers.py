"""Layer modules: the op compositions of the reference's model scripts, without
DGL.  Parameter names, shapes, initialisation and the order of ``B.*`` calls
follow the reference so that a state_dict and the kernel sequence line up:

  HET_RGATLayer                       hrt/python/RGAT/models.py:16-385
  HET_EglRelGraphConv_EdgeParallel    hrt/python/RGCN/RGCN.py:194-350
  HET_RelGraphEmbed                   hrt/python/RGNNUtils/RGNNUtils.py:78-119
  HET_HGTLayerHetero                  hrt/python/HGT/models.py:15-286
"""
from __future__ import annotations

import math

import os

import torch as th
import torch.nn as nn

from . import backend as B
from . import kernels as _k
from ._lib import HetError
from .backend import rgat_fused_layer as FL
from .backend import hgt_fused_layer as _hgt_fused
from .backend import hgt_route


PAD_HEADS = os.environ.get("HET_RGAT_PAD_HEADS", "1") != "0"  # zero-pad narrow / odd RGAT heads to the row kernels' widths
PAD_WIDTHS = os.environ.get("HET_PAD_WIDTHS", "1") != "0"     # zero-pad RGCN output widths to 32 / 64 / 128


def _needs_grad(x, module, *others) -> bool:
    """The ``grad`` fact of a call: autograd is on and the input, a parameter of the layer or one of ``others`` requires a gradient."""
    return th.is_grad_enabled() and any(t.requires_grad for t in (x, *others, *module.parameters()))


def _refuse_inference_graph(g, module, grad):
    """A graph whose tensors were created under ``torch.inference_mode()`` serves evaluation only: the autograd nodes save index
    tensors of the graph for their backward, and torch refuses to save an inference tensor.  A call that needs a gradient
    (``grad``: a bool, or a callable asked only for such a graph) is refused here, at the layer's entry, before any launch."""
    holds = getattr(g, "holds_inference_tensors", None)  # (a graph-like object without the method: nothing to ask, not refused)
    if holds is not None and holds() and (grad() if callable(grad) else grad):
        raise HetError(f"{type(module).__name__}: the graph's tensors were created in inference mode (torch.inference_mode()), so it "
                       "serves evaluation only: torch cannot save inference tensors for a backward.  Build the graph (and a "
                       "sampler and its blocks) outside inference mode to train on it; evaluation may run inside it")


def _padded_in_width(K: int) -> int:
    """Input width the matrix-core projections run with: 32 / 64 / 128.  Other widths up to 128 (16, 100 ...) run zero-padded --
    zero columns appended to the input rows and zero rows to every weight that multiplies them add nothing to any product; the
    padded columns of the input gradient are dropped by autograd.  One padded copy of the input per step (N x K' floats) against
    the any-shape GEMMs: ogbn-mag, 100 -> 64: RGAT 27 -> 7 ms, RGCN 35 -> 5 ms."""
    if not PAD_WIDTHS:
        return K
    return next((w for w in (32, 64, 128) if w >= K), K)


def _embed_rows_kernel_ok(embeds, nodes, dtype) -> bool:
    """Whether csrc/rows_embed.hip serves the gather: a contiguous, 16-byte aligned fp32 table on the GPU of a covered width, ids on
    the same device, float32 or bfloat16 rows out."""
    return (embeds.is_cuda and embeds.dtype == th.float32 and embeds.dim() == 2 and embeds.is_contiguous()
            and embeds.data_ptr() % 16 == 0 and nodes.device == embeds.device and dtype in (th.float32, th.bfloat16)
            and _k.rows_embed_ok(embeds.shape[1]))


def _embed_rows(embeds, nodes, dtype):
    """embeds[nodes] as [B, K] in ``dtype``: the gather kernel where it applies (bf16 rounded once at its store), else index_select and
    a cast -- correct, not fast."""
    if _embed_rows_kernel_ok(embeds, nodes, dtype):
        return _k.rows_embed_gather(embeds, nodes.contiguous(), dtype)
    return embeds.index_select(0, nodes).to(dtype)


class _EmbedRowsFunction(th.autograd.Function):
    """rows = embeds[nodes] as one autograd node that saves ``nodes`` only.  The gradient of the table is dense [N, K] (the values
    autograd's own index backward gives: zeros + index_put_(accumulate=True)) or, ``sparse``, the uncoalesced
    torch.sparse_coo_tensor(nodes, grad_out) that nn.Embedding(sparse=True) returns -- B rows instead of N."""

    @staticmethod
    def forward(ctx, embeds, nodes, dtype, sparse):
        ctx.save_for_backward(nodes)
        ctx.table_shape, ctx.sparse = embeds.shape, sparse
        return _embed_rows(embeds.detach(), nodes, dtype)

    @staticmethod
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        nodes, = ctx.saved_tensors
        vals = grad_out.detach().to(th.float32).contiguous()  # (a strided or expanded grad_out: read, never written)
        if ctx.sparse:
            if vals.data_ptr() == grad_out.data_ptr():
                vals = vals.clone()  # (grad_out may be shared with another branch: the gradient returned owns its values)
            return th.sparse_coo_tensor(nodes.reshape(1, -1), vals, ctx.table_shape), None, None, None
        grad = th.zeros(ctx.table_shape, dtype=th.float32, device=vals.device)
        grad.index_put_((nodes,), vals, accumulate=True)
        return grad, None, None, None


class HET_RelGraphEmbed(nn.Module):
    """Learnable node embeddings used as input features (RGNNUtils.py:78-119).

    ``forward()`` returns the whole table, as the reference does.  ``forward(nodes, dtype=None)`` returns ``embeds[nodes]`` as
    [B, K] rows in ``dtype`` (None: float32; torch.bfloat16: rounded once where the rows are stored) through one autograd node that
    saves ``nodes`` only -- what a sampled mini-batch needs of the table.  On a GPU table of a width that is a multiple of 4 up to
    1024 it is a HIP gather (csrc/rows_embed.hip); elsewhere (CPU, other widths, a non-contiguous table) index_select and a cast.

    ``sparse=True`` (opt-in): the gradient of ``forward(nodes)`` is a torch.sparse_coo_tensor of the B rows, uncoalesced, as
    nn.Embedding(sparse=True) gives -- no [N, K] zero-fill and scatter per step.  It takes an optimizer for sparse gradients:
    het_amd.optim.RowSparseAdam (one HIP launch per step) or torch.optim.SparseAdam.  ``forward()`` without nodes stays dense."""

    def __init__(self, num_nodes: int, embed_size: int, sparse: bool = False):
        super().__init__()
        self.sparse = bool(sparse)
        self.embeds = nn.Parameter(th.Tensor(num_nodes, embed_size))
        nn.init.xavier_uniform_(self.embeds)

    def forward(self, nodes=None, dtype=None):
        if nodes is None:
            return self.embeds if dtype is None or dtype == self.embeds.dtype else self.embeds.to(dtype)
        if nodes.dim() != 1 or nodes.dtype != th.int64:
            raise HetError(f"HET_RelGraphEmbed: nodes is a 1-d int64 tensor of row ids, got {tuple(nodes.shape)} {nodes.dtype}")
        return _EmbedRowsFunction.apply(self.embeds, nodes, self.embeds.dtype if dtype is None else dtype, self.sparse)


_M64 = (1 << 64) - 1


def _i64(v: int) -> int:
    """The 64 bits of ``v`` as a signed value (what an int64 tensor holds)."""
    return ((int(v) & _M64) ^ (1 << 63)) - (1 << 63)


def keyed_dropout_params(p: float):
    """(T, scale) of the keyed dropout rule (KeyedDropout) in plain Python: T = min(round-half-away(p * 65536), 65535), scale =
    65536 / (65536 - T) rounded once to float32 -- the values het_keyed_dropout_params gives."""
    import struct
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"keyed dropout: a rate in [0, 1), not {p}")
    x = p * 65536.0
    T = int(math.floor(x))
    if x - T >= 0.5:
        T += 1
    T = min(T, 65535)
    return T, struct.unpack("f", struct.pack("f", 65536.0 / (65536 - T)))[0]


def _lsr(z, k: int):
    """Logical right shift of an int64 tensor: the arithmetic shift with the copied sign bits masked off."""
    return (z >> k) & ((1 << (64 - k)) - 1)


def _sm_tensor(z):
    """sm of het_amd/sampling.py on an int64 tensor: the same 64 bits as the uint64 arithmetic (int64 add and multiply wrap)."""
    z = z + _i64(0x9E3779B97F4A7C15)
    z = (z ^ _lsr(z, 30)) * _i64(0xBF58476D1CE4E5B9)
    z = (z ^ _lsr(z, 27)) * _i64(0x94D049BB133111EB)
    return z ^ _lsr(z, 31)


def keyed_dropout_mask(seed: int, draw: int, base: int, n: int, p: float, device=None):
    """kept [n] (bool) of the keyed dropout rule in torch int64 arithmetic, on any device: the bits the kernels recompute."""
    from .sampling import _sm_int
    T, _ = keyed_dropout_params(p)
    if base < 0 or base % 4:
        raise ValueError(f"keyed dropout: base is a multiple of 4, at least 0, not {base}")
    stream = _sm_int((int(seed) & _M64) ^ _sm_int(int(draw) & _M64))
    groups = th.arange((n + 3) // 4, dtype=th.int64, device=device)
    key = _sm_tensor(groups + _i64(stream + base // 4))
    field = th.stack([(key >> (16 * j)) & 0xFFFF for j in range(4)], dim=1).reshape(-1)[:n]
    return field >= T


def _keyed_dropout_torch(y, p, seed, draw, base, relu):
    """The rule as a torch composition in fp32, cast back: correct, not fast (CPU tensors, other dtypes, strided or misaligned ones)."""
    _, scale = keyed_dropout_params(p)
    kept = keyed_dropout_mask(seed, draw, base, y.numel(), p, y.device).view(y.shape)
    v = y.to(th.float32)
    if relu:
        v = th.where(v < 0, th.zeros_like(v), v)  # (not th.relu: a NaN stays a NaN and -0 stays -0, as the kernel's select does)
    return th.where(kept, v * scale, th.zeros_like(v)).to(y.dtype)


def _keyed_dropout_backward_torch(grad_out, out, p, seed, draw, base, relu):
    _, scale = keyed_dropout_params(p)
    kept = keyed_dropout_mask(seed, draw, base, grad_out.numel(), p, grad_out.device).view(grad_out.shape)
    if relu:
        kept = kept & (out > 0)
    g = grad_out.to(th.float32)
    return th.where(kept, g * scale, th.zeros_like(g)).to(grad_out.dtype)


class _KeyedDropoutFunction(th.autograd.Function):
    """out = drop(a(y)) as one autograd node that keeps (p, seed, draw, base) of its own call and saves ``out`` for relu, nothing
    for the identity: the mask is recomputed from the key in the backward.  One HIP launch each way where the kernels take the
    tensors (csrc/keyed_dropout.hip), the torch composition with the same mask bits elsewhere."""

    @staticmethod
    def forward(ctx, y, p, seed, draw, base, relu):
        ctx.key = (float(p), int(seed), int(draw), int(base), bool(relu))
        yd = y.detach()
        out = _k.keyed_dropout(yd, p, seed, draw, relu, base) if _k.keyed_dropout_ok(yd) else _keyed_dropout_torch(yd, p, seed, draw, base, relu)
        if relu:
            ctx.save_for_backward(out)
        return out

    @staticmethod
    @th.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0] or grad_out is None:
            return None, None, None, None, None, None
        p, seed, draw, base, relu = ctx.key
        out = ctx.saved_tensors[0] if relu else None
        go = grad_out.detach().contiguous()  # (an expanded or strided grad_out: read, never written)
        if _k.keyed_dropout_ok(*((go, out) if relu else (go,))):
            grad_y = _k.keyed_dropout_backward(go, out, p, seed, draw, relu, base)
        else:
            grad_y = _keyed_dropout_backward_torch(go, out, p, seed, draw, base, relu)
        return grad_y, None, None, None, None, None


class KeyedDropout(nn.Module):
    """Dropout whose mask is a pure function of (seed, draw, position), fused with the activation that precedes it: ``out =
    drop(a(y))`` in one pass, its backward in one pass, no mask stored (opt-in).

    **A different sample than nn.Dropout's for the same torch seed**, with the same distribution.  All arithmetic is uint64 and wraps;
    ``sm`` is the keyed sampler's (het_amd/sampling.py); ``i`` is the element's index in the contiguous tensor::

        T      = min(round(p * 65536), 65535)       the effective rate is T / 65536 (0.5 is exact)
        scale  = float32(65536 / (65536 - T))
        stream = sm(seed ^ sm(draw))
        key(g) = sm(stream + g)                     g = i // 4: one key per 4 consecutive elements
        field  = (key(g) >> (16 * (i % 4))) & 0xFFFF
        kept   = field >= T
        out[i]    = a(y[i]) * scale if kept else +0             a = identity, or y < 0 ? 0 : y ("relu")
        grad_y[i] = grad_out[i] * scale if kept and (a is the identity or out[i] > 0) else +0

    bf16 tensors are widened, multiplied in fp32 and rounded once; every output is determined to the bit, on every device.

    ``seed=None`` draws the seed once, at construction, from torch's default CPU generator (deterministic under
    ``torch.manual_seed``).  ``draw`` is a counter of the module: 0 at first, one more per training call that drops something, so
    that successive steps use different streams; ``forward(y, draw=)`` sets it for one call and leaves the counter alone (the
    sampler's convention).  The autograd node of a call keeps that call's own (seed, draw).

    In training with p > 0, a contiguous, aligned float32 / bfloat16 GPU tensor takes the HIP kernels; everything else (CPU tensors,
    other dtypes, non-contiguous or misaligned inputs) takes a torch composition that produces the same mask bits in fp32, cast
    back: correct, not fast.  In ``eval()``, or when nothing would be dropped (T = 0), the module is the activation alone in torch
    and the counter does not move."""

    def __init__(self, p: float = 0.5, activation=None, seed=None):
        super().__init__()
        if activation not in (None, "relu"):
            raise ValueError(f"KeyedDropout: activation None or 'relu', not {activation!r}")
        self.T, self.scale = keyed_dropout_params(p)
        self.p, self.activation = float(p), activation
        self.seed = int(th.randint(0, 2 ** 63 - 1, (1,))) if seed is None else int(seed) & _M64
        self.draw = 0

    def extra_repr(self):
        return f"p={self.p}, activation={self.activation!r}"

    def forward(self, y, draw=None):
        if not self.training or self.T == 0:
            return th.relu(y) if self.activation == "relu" else y
        if draw is None:
            draw, self.draw = self.draw, self.draw + 1
        return _KeyedDropoutFunction.apply(y, self.p, self.seed, int(draw), 0, self.activation == "relu")


def _activation_dropout(layer, h):
    """The end of an RGAT / RGCN layer: ``dropout(activation(h))`` -- two torch ops, or with ``keyed_dropout=True`` one KeyedDropout
    call (relu inside it; any other activation applied in torch first)."""
    if not layer.keyed_dropout:
        if layer.activation:
            h = layer.activation(h)
        return layer.dropout(h)
    if layer.activation and layer.dropout.activation is None:
        h = layer.activation(h)
    return layer.dropout(h if h.is_contiguous() else h.contiguous())  # (a sliced padded width: one copy instead of the composition)


def _make_dropout(layer, dropout, keyed_dropout):
    """nn.Dropout, or (``keyed_dropout=True``, opt-in) KeyedDropout with relu fused where the layer's activation is relu."""
    layer.keyed_dropout = bool(keyed_dropout)
    if not layer.keyed_dropout:
        return nn.Dropout(dropout)
    return KeyedDropout(dropout, "relu" if layer.activation in (th.relu, nn.functional.relu) else None)


def _xent_rows(z, labels, ignore_index):
    """(valid [N] bool, bad [N] bool, label-or-0 [N]) of the cross-entropy rule: a label is used as an index only where it is valid."""
    valid = (labels != ignore_index) & (labels >= 0) & (labels < z.shape[1])
    return valid, (labels != ignore_index) & ~valid, th.where(valid, labels, th.zeros_like(labels))


def _softmax_xent_torch(z, labels, ignore_index, reduction, want_lse):
    """The rule of SoftmaxCrossEntropy as a torch composition (fp32; fp64 logits in fp64): (loss, lse or None, stats).  Correct, not
    fast: CPU tensors, other dtypes, non-contiguous or misaligned logits."""
    acc = th.float64 if z.dtype == th.float64 else th.float32
    zf = z.to(acc)
    valid, bad, lab = _xent_rows(zf, labels, ignore_index)
    m = zf.max(dim=1).values
    lsum = th.log(th.exp(zf - m[:, None]).sum(dim=1))  # (a row of -inf, a NaN, +inf: NaN, as the kernels give)
    zl = zf.gather(1, lab[:, None]).squeeze(1)
    zero = th.zeros((), dtype=acc, device=z.device)
    row_loss = th.where(valid, lsum + (m - zl), zero)
    total = row_loss.double().sum()
    n_valid = valid.sum()
    loss = (total / n_valid if reduction == "mean" else total).to(th.float32 if acc == th.float32 else acc)
    # correct: the label's logit is the first of the row's maxima, a NaN above everything (torch.argmax on the CPU, on any device)
    lower = th.arange(zf.shape[1], device=z.device)[None, :] < lab[:, None]
    nan, zlc = zf.isnan(), zl[:, None]
    beaten = th.where(zl.isnan()[:, None], nan & lower, nan | (zf > zlc) | ((zf == zlc) & lower)).any(dim=1)
    stats = th.stack([n_valid, (valid & ~beaten).sum(), bad.sum()]).to(th.int64)
    return loss, (th.where(valid, m + lsum, zero) if want_lse else None), stats


def _softmax_xent_backward_torch(z, labels, lse, stats, grad_loss, ignore_index, reduction):
    acc = lse.dtype
    valid, _, lab = _xent_rows(z, labels, ignore_index)
    gs = grad_loss.to(acc) / stats[0].to(acc) if reduction == "mean" else grad_loss.to(acc)
    p = th.exp(z.to(acc) - lse[:, None])
    p = p - th.nn.functional.one_hot(lab, z.shape[1]).to(acc)
    return th.where(valid[:, None], p * gs, th.zeros((), dtype=acc, device=z.device)).to(z.dtype)


class SoftmaxCrossEntropyFunction(th.autograd.Function):
    """(loss, stats) = softmax cross-entropy of ``logits`` [N, C] against ``labels`` [N] as one autograd node: one HIP launch and a
    one-wave finish forward, one launch backward where the kernels take the tensors (csrc/softmax_xent.hip), the torch composition
    of the same rule elsewhere.  Saved for the backward: the logits, the labels, lse [N] and stats -- nothing else of size [N, C];
    nothing when ``logits`` needs no gradient.  ``stats`` (int64 [3]: valid, correct, bad rows) is not differentiable."""

    @staticmethod
    def forward(ctx, logits, labels, ignore_index, reduction):
        z, lab = logits.detach(), labels.detach()
        if lab.dtype != th.int64:
            lab = lab.to(th.int64)
        want = ctx.needs_input_grad[0]
        ctx.rule = (int(ignore_index), reduction)
        ctx.native = _k.softmax_xent_ok(z, lab)
        if ctx.native:
            if reduction not in _k.XENT_REDUCTIONS:
                raise HetError(f"SoftmaxCrossEntropyFunction: reduction 'mean' or 'sum', not {reduction!r}")
            loss, lse, stats = _k._softmax_xent(z, lab, int(ignore_index), reduction, want)
        else:
            loss, lse, stats = _softmax_xent_torch(z, lab, int(ignore_index), reduction, want)
        if want:
            ctx.save_for_backward(z, lab, lse, stats)
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)  # (no zero-filled int64 [3] made and launched per backward for the gradient stats never has)
        return loss, stats

    @staticmethod
    @th.autograd.function.once_differentiable
    def backward(ctx, grad_loss, _grad_stats):
        if not ctx.needs_input_grad[0] or grad_loss is None:
            return None, None, None, None
        z, lab, lse, stats = ctx.saved_tensors
        ignore_index, reduction = ctx.rule
        g = grad_loss.detach().to(device=z.device, dtype=lse.dtype).contiguous()  # (read on the device, never written)
        if ctx.native:
            return _k._softmax_xent_backward(z, lab, lse, stats, g, ignore_index, reduction), None, None, None
        return _softmax_xent_backward_torch(z, lab, lse, stats, g, ignore_index, reduction), None, None, None


class SoftmaxCrossEntropy(nn.Module):
    """Softmax cross-entropy of ``logits`` [N, C] against integer ``labels`` [N] as one pass each way (opt-in): what
    ``F.cross_entropy(logits, labels, ignore_index=, reduction=)`` computes, with two deliberate differences.

    * A label that is neither ``ignore_index`` nor in [0, C) does not assert on the device: its row is skipped like an ignored one
      and counted (``last_stats[2]``).  ``check_labels=True`` reads that count back after every call -- the module's only host
      synchronisation -- and raises ValueError naming it.
    * The loss is summed in fp64 in a fixed order, without float atomics: the same inputs give the same bits on every call.

    Per valid row, in fp32 (bf16 logits widened first): ``m = max z``, ``lse = m + log(sum(exp(z - m)))``, ``loss_i = lse - z[label]``;
    ``reduction="mean"`` divides the sum by the number of valid rows, counted on the device (none: NaN, and a gradient of zeros);
    ``grad[i, c] = (exp(z_c - lse_i) - [c == label_i]) * g * (1 or 1 / valid)`` in the logits' dtype, +0 in skipped rows.

    ``forward`` returns the fp32 scalar loss.  ``last_stats`` is the int64 device tensor (valid rows, rows whose argmax is the label,
    bad rows) of the last call; ``accuracy()`` is correct / valid as a device tensor.  Ignored labels take the place of indexing the
    logits with a training / validation subset: no gather, and no index-put into a zero-filled [N, C] in the backward.

    Contiguous, aligned float32 / bfloat16 GPU logits take the HIP kernels; everything else (CPU tensors, fp16 / fp64, non-contiguous
    or misaligned logits) takes a torch composition of the same rule: correct, not fast.  Labels of another integer type are cast."""

    def __init__(self, ignore_index: int = -100, reduction: str = "mean", check_labels: bool = False):
        super().__init__()
        if reduction not in _k.XENT_REDUCTIONS:
            raise ValueError(f"SoftmaxCrossEntropy: reduction 'mean' or 'sum', not {reduction!r}")
        self.ignore_index, self.reduction, self.check_labels = int(ignore_index), reduction, bool(check_labels)
        self.last_stats = None

    def extra_repr(self):
        return f"ignore_index={self.ignore_index}, reduction={self.reduction!r}, check_labels={self.check_labels}"

    def forward(self, logits, labels):
        if logits.dim() != 2 or labels.dim() != 1 or labels.shape[0] != logits.shape[0] or logits.shape[1] < 1:
            raise ValueError(f"SoftmaxCrossEntropy: logits [N, C] with C >= 1 and labels [N], got {tuple(logits.shape)} and {tuple(labels.shape)}")
        if labels.is_floating_point() or labels.dtype == th.bool:
            raise ValueError(f"SoftmaxCrossEntropy: integer class labels, not {labels.dtype}")
        loss, stats = SoftmaxCrossEntropyFunction.apply(logits, labels, self.ignore_index, self.reduction)
        self.last_stats = stats
        if self.check_labels:
            bad = int(stats[2])
            if bad:
                raise ValueError(f"SoftmaxCrossEntropy: {bad} label(s) are neither ignore_index ({self.ignore_index}) nor in "
                                 f"[0, {logits.shape[1]})")
        return loss

    def accuracy(self):
        """correct / valid of the last call, as a device tensor (NaN when no row was valid)."""
        if self.last_stats is None:
            raise HetError("SoftmaxCrossEntropy.accuracy(): no call yet")
        return self.last_stats[1].to(th.float32) / self.last_stats[0].to(th.float32)


class HET_RGATLayer(nn.Module):
    """Relational graph attention layer (RGAT/models.py:16-385).

    Which code serves a call -- the one-node layer and its evaluation forms, the op-by-op composition below, the reference's op
    sequence, or the fp32 layer on an upcast copy -- is decided in one place: the table in het_amd/backend/rgat_route.py.

    bf16 activations: a ``torch.bfloat16`` input gives a bf16 output.  Where the call runs natively in bf16 (evaluation on one GPU:
    path ``eval_bf16`` of that table), x, the projected rows feat_c and the output rows are bf16, each rounded once where its kernel
    stores it; the parameters, el / er, the softmax and every sum stay fp32 (het_amd/backend/rgat_fused_layer.py); er always comes
    from the folded weight.  Every other bf16 call (``upcast``) runs the fp32 layer on ``x.float()`` and casts the result; autograd
    casts the gradient of the input back to bf16.  That fallback is correct, not faster.

    ``bf16_training=True`` (opt-in; the default keeps the upcast for every call that needs a gradient): where the table has
    ``train_bf16``, a bf16 input that requires a gradient, or a layer whose parameters do, trains natively in bf16 -- the same
    forward with the training aggregation, and a backward that gathers the bf16 gradient of the output, keeps every gradient sum and
    parameter gradient in fp32 and rounds the input gradient once (rgat_fused_layer.RgatLayerBf16Function) -- with or without the
    self-loop and the bias, on full graphs and blocks.  Evaluation calls and fp32 inputs are the same with either value.

    Attention weights: ``forward(..., get_attention=True)`` returns ``(h, attn)`` -- attn [E, num_heads] float32, detached, row i the
    softmax weight of the edge with id i (the graph's eids, whatever order the edges are stored in) among the in-edges of its
    destination; every row is filled, on a block too.  On the evaluation paths (fp32 and bf16) a HIP pass over the ids and the el /
    er tables writes them after the aggregation (csrc/gat_attention.hip); every other call gets them from a plain torch composition
    in fp32 under no_grad (rgat_fused_layer.attention_composition): correct, not fast.  No gradient flows through attn."""

    def __init__(self, in_feat, out_feat, num_rels, num_heads, *, bias=True, activation=None, self_loop=False,
                 compact_as_of_node_flag=False, compact_direct_indexing_flag=False,
                 multiply_among_weights_first_flag=False, gat_edge_parallel_flag=True, dropout=0.5,
                 leaky_relu_slope=0.2, reference_op_sequence=False, bf16_training=False, keyed_dropout=False):
        super().__init__()
        assert out_feat % num_heads == 0, "out_feat must be a multiple of num_heads"
        self.in_feat, self.out_feat, self.num_rels, self.num_heads = in_feat, out_feat, num_rels, num_heads
        self.bias, self.activation, self.self_loop = bias, activation, self_loop
        self.compact_as_of_node_flag = compact_as_of_node_flag
        self.compact_direct_indexing_flag = compact_direct_indexing_flag
        self.multiply_among_weights_first_flag = multiply_among_weights_first_flag
        self.gat_edge_parallel_flag = gat_edge_parallel_flag
        self.leaky_relu_slope = leaky_relu_slope
        self.bf16_training = bool(bf16_training)  # a bf16 input that needs a backward: natively where covered (the class docstring)
        # True: run the reference's op sequence literally (only reference-named torch_hrt ops, the reference wrappers'
        # zero-filled "+=" buffers; het_amd/backend/reference_protocol.py) -- the drop-in path bench.py times as
        # variants.reference_op_sequence.  Non-compact flags, full graph.
        self.reference_op_sequence = reference_op_sequence
        # True (or HET_RGAT_FUSED=0): the reference's model code line by line on this package's backend wrappers (het_amd.backend:
        # same function names as hrt/python/backend, buffers allocated without fills, "=" gradients) instead of the one-node layer --
        # what a reference checkout gets when it imports het_amd.backend in place of its own backend package
        self.op_by_op = os.environ.get("HET_RGAT_FUSED", "1") == "0"
        self.conv_weights = nn.Parameter(th.Tensor(num_rels, num_heads, in_feat, out_feat // num_heads))
        self.attn_l = nn.Parameter(th.Tensor(num_rels, num_heads, out_feat // num_heads))
        self.attn_r = nn.Parameter(th.Tensor(num_rels, num_heads, out_feat // num_heads))
        if bias:
            self.h_bias = nn.Parameter(th.Tensor(out_feat))
        if self_loop:
            self.loop_weight = nn.Parameter(th.Tensor(in_feat, out_feat))
        self.dropout = _make_dropout(self, dropout, keyed_dropout)
        self.reset_parameters()

    def reset_parameters(self):
        gain = nn.init.calculate_gain("relu")
        if self.bias:
            nn.init.zeros_(self.h_bias)
        if self.self_loop:
            nn.init.xavier_uniform_(self.loop_weight, gain=gain)
        nn.init.xavier_uniform_(self.conv_weights, gain=gain)
        nn.init.xavier_uniform_(self.attn_l, gain=gain)
        nn.init.xavier_uniform_(self.attn_r, gain=gain)

    def _w_attn_r(self):
        dk = self.out_feat // self.num_heads
        return th.bmm(self.conv_weights.view(-1, self.in_feat, dk), self.attn_r.view(-1, dk, 1)).view(
            -1, self.num_heads, self.in_feat, 1)

    def forward_with_halo(self, g, x_own: th.Tensor, halo):
        """Multi-GPU form (het_amd/dist.py): ``g`` is this rank's local graph (owned nodes first, then halo nodes), ``x_own``
        the features of the owned nodes; the layer runs the halo exchange itself (``halo``: a dist.HaloContext) and overlaps
        it with the work that needs owned rows only.  Returns the owned rows, or None when the one-node path does not
        cover the configuration (the caller then exchanges first and calls forward)."""
        return self._forward(g, x_own, x_own.shape[0], halo=halo)

    def _route(self, g, x, num_dst, halo):
        """Which code serves the call: the facts rgat_route.decide reads (its Facts) and its answer."""
        lists, dst_below, attn_dot_only = FL.graph_facts(g, x)
        facts = FL.rgat_route.Facts(
            cuda=x.is_cuda, bf16=x.dtype == th.bfloat16, dim=x.dim(), N=g.get_num_nodes() if halo else x.shape[0], K=self.in_feat, H=self.num_heads,
            D=self.out_feat // self.num_heads, R=self.num_rels, K_padded=_padded_in_width(self.in_feat), edges=g.get_num_edges() > 0,
            slope=self.leaky_relu_slope, grad=_needs_grad(x, self),
            halo=halo, num_dst=num_dst, plan=FL.rgat_layer_fused_ok(), lists=lists, compact_flag=self.compact_as_of_node_flag,
            direct_flag=self.compact_direct_indexing_flag, mulfirst_flag=self.multiply_among_weights_first_flag,
            gat_edge_parallel=self.gat_edge_parallel_flag, reference_op_sequence=self.reference_op_sequence, op_by_op=self.op_by_op,
            self_loop=self.self_loop, bf16_training=self.bf16_training, per_edge=FL.PER_EDGE, literal_er=FL.LITERAL_ER,
            forward_only=FL.FORWARD_ONLY, pad_heads=PAD_HEADS)
        _refuse_inference_graph(g, self, facts.grad)
        return FL.rgat_route.decide(facts, dst_below, attn_dot_only)

    def _fused(self, route, g, inputs, num_dst, halo, attn_out):
        """The one-node layer (het_amd/backend/rgat_fused_layer.py) at the widths of ``route``: same ops and values as the
        composition, gradients of the shared input accumulated in place instead of summed by autograd.
        Narrow outputs -- the reference's own RGAT experiment is 128 -> 8 classes over 8 heads, one float per head
        (hrt/experiments/run_het_rgat.sh) -- and heads whose width is not a power of two are outside the row kernels (4+ floats per
        head, 32+ per row for the matrix-core projection).  Zero-padding every head to D' changes no value: the padded columns of W,
        attn_l, attn_r, the self-loop weight and the bias are zero, so el / er, the softmax and the first D components of every head
        are the same sums and the padded output components are zero (dropped below); the gradients of the padding are dropped by
        autograd.  HET_RGAT_PAD_HEADS=0: off (op-by-op composition / any-shape kernels as before)."""
        H, D, K = self.num_heads, self.out_feat // self.num_heads, self.in_feat
        Kp, Dp = route.Kp, route.Dp
        x, W, al, ar = inputs, self.conv_weights, self.attn_l, self.attn_r
        loop, bias = self.loop_weight if self.self_loop else None, self.h_bias if self.bias else None
        if (Kp, Dp) != (K, D):
            pad = (0, Dp - D)
            x = nn.functional.pad(inputs, (0, Kp - K)) if Kp != K else inputs
            W = nn.functional.pad(W, pad + (0, Kp - K))
            al, ar = nn.functional.pad(al, pad), nn.functional.pad(ar, pad)
            loop = nn.functional.pad(loop.view(K, H, D), pad + (0, 0, 0, Kp - K)).view(Kp, H * Dp) if self.self_loop else None
            bias = nn.functional.pad(bias.view(H, D), pad).view(H * Dp) if self.bias else None
        h = FL.rgat_layer_fused(route, g, x, W, al, ar, loop, bias, self.leaky_relu_slope, num_dst, halo=halo, attn_out=attn_out)
        if (Kp, Dp) != (K, D):
            h = h.view(h.shape[0], H, Dp)[:, :, :D].reshape(h.shape[0], self.out_feat)
        return h

    def forward(self, g, inputs: th.Tensor, num_dst=None, get_attention=False):
        """``num_dst``: the destination nodes of ``g`` are its first ``num_dst`` nodes (a sampled block, or the owned
        nodes of a partition followed by halo nodes): only their rows are returned and the self-loop runs on them only.
        ``get_attention``: return ``(h, attn)``, attn [E, num_heads] float32 in edge-id order (the class docstring)."""
        if not get_attention:
            return self._forward(g, inputs, num_dst)
        attn_out = []
        h = self._forward(g, inputs, num_dst, attn_out)
        if not attn_out:  # the call did not take an evaluation path: correct, not fast
            attn_out.append(FL.attention_composition(g, inputs, self.conv_weights, self.attn_l, self.attn_r, self.leaky_relu_slope))
        return h, attn_out[0]

    def _forward(self, g, inputs, num_dst=None, attn_out=None, halo=None):
        """forward and forward_with_halo; ``attn_out`` (a list): where the call takes an evaluation path, the attention weights are
        appended to it."""
        route = self._route(g, inputs, num_dst, halo is not None)
        if route.path == "upcast":  # correct, not faster: the fp32 layer on an upcast copy (autograd casts the gradient of the input)
            h = self._forward(g, inputs.float(), num_dst, attn_out, halo)
            return None if h is None else h.to(th.bfloat16)
        if halo is not None and route.path != "node":
            return None
        if route.path == "reference":
            assert not self.compact_as_of_node_flag and num_dst is None and self.gat_edge_parallel_flag
            from .backend.reference_protocol import rgat_layer_reference_sequence
            return rgat_layer_reference_sequence(self, g, inputs)
        if route.path == "composition":
            h = self._composition(g, inputs, num_dst)
        else:
            h = self._fused(route, g, inputs, num_dst, halo, attn_out)
        return _activation_dropout(self, h)

    def _composition(self, g, inputs, num_dst):
        """The reference's model code op by op on this package's backend wrappers, up to and including the bias."""
        if self.compact_as_of_node_flag:  # models.py:152-263
            ss, d_row, d_col = FL._unique_lists(g)
            feat_compact = B.rgnn_relational_matmul(d_row, self.conv_weights, inputs, True, 1)
            fuse_el = self.gat_edge_parallel_flag and B.relational_fused_gat_compact_with_attn_l_ok(
                g, feat_compact, self.attn_l, self.leaky_relu_slope)
            if not fuse_el:
                el_compact = B.rgnn_relational_matmul_no_scatter_gather_list(
                    ss["rel_ptrs_row"], self.attn_l.unsqueeze(-1), feat_compact)
            if self.multiply_among_weights_first_flag:
                er_compact = B.rgnn_relational_matmul(d_col, self._w_attn_r(), inputs, True, 1)
            else:
                feat_compact_dst = B.rgnn_relational_matmul(d_col, self.conv_weights, inputs, True, 1)
                er_compact = B.rgnn_relational_matmul_no_scatter_gather_list(
                    ss["rel_ptrs_col"], self.attn_r.unsqueeze(-1), feat_compact_dst)
            if not self.gat_edge_parallel_flag:
                raise NotImplementedError("single-sided unique node lists need the edge-parallel op (models.py:253-256)")
            if fuse_el:  # el and the GAT op under one autograd node (same values, one gradient store for feat_compact)
                h = B.relational_fused_gat_compact_with_attn_l(
                    g, feat_compact, self.attn_l, er_compact.view(er_compact.shape[0], self.num_heads),
                    self.leaky_relu_slope, self.compact_direct_indexing_flag)
            else:
                h = B.relational_fused_gat_compact_as_of_node_separate_coo_single_sided(
                    g, feat_compact, el_compact.view(el_compact.shape[0], self.num_heads),
                    er_compact.view(er_compact.shape[0], self.num_heads), self.leaky_relu_slope,
                    self.compact_direct_indexing_flag)
        else:  # models.py:265-372
            s, by_src, by_dst = FL._lists(g)
            by_eid = {"separate_coo_rel_ptrs": s["rel_ptrs"], "separate_coo_node_indices": s["eids"],
                      "separate_coo_eids": s["eids"]}
            # Same values as the reference's op sequence, fewer passes over the [E,H,D] tensors where the shapes
            # allow: the attention terms el / er come out of the projection GEMM's epilogue (dot_ok), and el and the
            # GAT op share one autograd node (fuse_el) so the two gradients of feat_src_per_edge are written by one store
            dot_ok = B.rgnn_relational_matmul_with_attn_dot_ok(self.conv_weights, inputs)
            fuse_el = self.gat_edge_parallel_flag and inputs.is_cuda and B.relational_fused_gat_separate_coo_with_attn_l_ok(
                g, inputs, self.attn_l, self.leaky_relu_slope)
            el = None
            if dot_ok:
                feat_src_per_edge, el = B.rgnn_relational_matmul_with_attn_dot(by_src, self.conv_weights, inputs,
                                                                               self.attn_l, folded=fuse_el)
            else:
                feat_src_per_edge = B.rgnn_relational_matmul(by_src, self.conv_weights, inputs, True, 0)
                if not fuse_el:
                    el = B.rgnn_relational_matmul(by_eid, self.attn_l.unsqueeze(-1), feat_src_per_edge, False, 0)
            if self.multiply_among_weights_first_flag:
                # one input head, [R,H,K,1] weight (the reference passes False here, models.py:310-326,
                # which only works for num_heads == 1)
                er = B.rgnn_relational_matmul(by_dst, self._w_attn_r(), inputs, True, 0)
            elif dot_ok and B.rgnn_relational_matmul_attn_dot_only_ok(by_dst, self.conv_weights, inputs):
                # the per-edge projection by destination feeds nothing but er: it is not materialised
                er = B.rgnn_relational_matmul_attn_dot_only(by_dst, self.conv_weights, inputs, self.attn_r)
            elif dot_ok:
                _, er = B.rgnn_relational_matmul_with_attn_dot(by_dst, self.conv_weights, inputs, self.attn_r)
            else:
                feat_dst_per_edge = B.rgnn_relational_matmul(by_dst, self.conv_weights, inputs, True, 0)
                er = B.rgnn_relational_matmul(by_eid, self.attn_r.unsqueeze(-1), feat_dst_per_edge, False, 0)
            er = er.view(-1, self.num_heads)
            if fuse_el:
                h = B.relational_fused_gat_separate_coo_with_attn_l(g, feat_src_per_edge, self.attn_l, er,
                                                                    self.leaky_relu_slope, el=el)
            elif self.gat_edge_parallel_flag:
                el = el.view(-1, self.num_heads)
                h = B.relational_fused_gat_separate_coo(g, feat_src_per_edge, el, er, self.leaky_relu_slope)
            else:
                h = B.relational_fused_gat_csr(g, feat_src_per_edge, el.view(-1, self.num_heads), er, self.leaky_relu_slope)
        h = h.view(-1, self.out_feat)  # models.py:377-385
        loop_in = inputs
        if num_dst is not None and num_dst < inputs.shape[0]:
            h, loop_in = h[:num_dst], inputs[:num_dst]
        if self.self_loop:
            # the reference calls th.matmul here (models.py:378-379); same product through the segment GEMM
            # with a single segment (MFMA kernel instead of a generic BLAS pick for a 64-wide GEMM)
            h = h + B.rgnn_relational_matmul_no_scatter_gather_list(
                FL._loop_offsets(loop_in.shape[0], inputs.device), self.loop_weight.view(1, 1, self.in_feat, self.out_feat), loop_in)
        return h + self.h_bias if self.bias else h


class HET_EglRelGraphConv_EdgeParallel(nn.Module):
    """RGCN layer on the fused separate-COO op (RGCN/RGCN.py:194-350).

    bf16 activations: a ``torch.bfloat16`` input gives a bf16 output (and a bf16 input gradient); the parameters, their
    gradients, the edge norm and every sum stay fp32.  Where the two-call layer applies (groupings on, a shape of
    kernels.rgcn_layer_ok, output width 32 or 64 after padding, HET_RGCN_FUSED on, not compact_as_of_node_flag) the library's
    bf16 entries run and the bias, zero-padded to a padded width, is added inside them, so the output is rounded once.  Every
    other path -- compact_as_of_node_flag, groupings off (plan.forced(False): one-shot block graphs), shapes outside
    rgcn_layer_ok such as 8 relations at 64 x 64, HET_RGCN_FUSED=0, widths padded to 128 -- runs the fp32 layer on an upcast copy
    of the input and rounds its output to bf16: correct, not faster, and it needs the fp32 copy.

    ``regularizer="bdd"`` (DGL's RelGraphConv; RGCN/RGCN.py names it): ``num_bases`` = B diagonal blocks per relation, ``weight``
    [num_rels, B, in_feat / B, out_feat / B], no ``w_comp``; B must divide both widths (ValueError).  A call is served by the
    block kernels (csrc/rgcn_bdd.hip) or by this layer's existing code on the dense expansion of the blocks, as
    backend.rgcn_bdd_route decides; ``last_route`` is "native" or "dense" after every call."""

    def __init__(self, in_feat, out_feat, num_rels, num_bases=-1, *, bias=True, activation=None,
                 compact_as_of_node_flag=False, compact_direct_indexing_flag=False, dropout=0.0, keyed_dropout=False,
                 regularizer="basis"):
        super().__init__()
        if regularizer not in ("basis", "bdd"):
            raise ValueError("Regularizer must be either 'basis' or 'bdd'")  # (RGCN/RGCN.py)
        self.in_feat, self.out_feat, self.num_rels, self.regularizer = in_feat, out_feat, num_rels, regularizer
        self.bias, self.activation = bias, activation
        self.compact_as_of_node_flag = compact_as_of_node_flag
        self.compact_direct_indexing_flag = compact_direct_indexing_flag
        self._upcast_of_bf16 = False
        self.last_route = None  # "native" / "dense" of the last bdd call (backend: rgcn_bdd_route); None for the basis regularizer
        gain = nn.init.calculate_gain("relu")
        if regularizer == "bdd":
            # DGL's RelGraphConv(regularizer="bdd"): num_bases diagonal blocks of [in_feat / B, out_feat / B] per relation, no w_comp
            if num_bases < 1 or in_feat % num_bases != 0 or out_feat % num_bases != 0:
                raise ValueError(f"Feature size must be a multiplier of num_bases ({num_bases}): got {in_feat} -> {out_feat}")
            self.num_bases = num_bases
            self.weight = nn.Parameter(th.Tensor(num_rels, num_bases, in_feat // num_bases, out_feat // num_bases))
            nn.init.xavier_uniform_(self.weight, gain=gain)
            if bias:
                self.h_bias = nn.Parameter(th.zeros(out_feat))
            self.dropout = _make_dropout(self, dropout, keyed_dropout)
            return
        self.num_bases = num_rels if num_bases <= 0 or num_bases > num_rels else num_bases
        self.weight = nn.Parameter(th.Tensor(self.num_bases, in_feat, out_feat))
        nn.init.xavier_uniform_(self.weight, gain=gain)
        if self.num_bases < num_rels:
            self.w_comp = nn.Parameter(th.Tensor(num_rels, self.num_bases))
            nn.init.xavier_uniform_(self.w_comp, gain=gain)
        if bias:
            self.h_bias = nn.Parameter(th.zeros(out_feat))
        self.dropout = _make_dropout(self, dropout, keyed_dropout)

    def forward(self, g, x, norm, num_dst=None):
        _refuse_inference_graph(g, self, lambda: _needs_grad(x, self, norm))
        if self.regularizer == "bdd" and not self._upcast_of_bf16:
            bias = self.h_bias if self.bias else None
            self.last_route = B.rgcn_bdd_route_of(g, x, self.weight, norm, bias, self.compact_as_of_node_flag)
            if self.last_route == "native":  # (the bias inside the op; the destinations' rows are sliced afterwards)
                node_repr = B.rgcn_layer_bdd(g, x, self.weight, norm, bias)
                if num_dst is not None and num_dst < node_repr.shape[0]:
                    node_repr = node_repr[:num_dst]
                return _activation_dropout(self, node_repr)
        if x.dtype == th.bfloat16:
            return self._forward_bf16(g, x, norm, num_dst)
        weight, x = self._weight_and_input(x)
        if self.compact_as_of_node_flag:  # RGCN.py:310-336
            ss = g.get_separate_unique_node_indices_single_sided()
            d_row = {"unique_srcs_and_dests_rel_ptrs": ss["rel_ptrs_row"],
                     "unique_srcs_and_dests_node_indices": ss["node_indices_row"]}
            feat_compact = B.rgnn_relational_matmul(d_row, weight.unsqueeze(1), x, True, 1)
            node_repr = B.rgcn_node_mean_aggregation_compact_as_of_node_separate_coo_single_sided(
                g, feat_compact.view(feat_compact.shape[0], -1), norm, self.compact_direct_indexing_flag)
        else:
            # (the bias joins the op's output buffer when all rows are kept: backend RgcnLayer1SeparateCooBias)
            bias_in_op = self.bias and (num_dst is None or num_dst >= g.get_num_nodes()) and weight.shape[2] == self.out_feat
            node_repr = B.rgcn_layer1_separate_coo(g, x, weight, norm, self.h_bias if bias_in_op else None)
            if bias_in_op:
                return _activation_dropout(self, node_repr)
        if num_dst is not None and num_dst < node_repr.shape[0]:
            node_repr = node_repr[:num_dst]
        if node_repr.shape[1] != self.out_feat:  # (padded widths: see above)
            node_repr = node_repr[:, :self.out_feat]
        if self.bias:
            node_repr = node_repr + self.h_bias
        return _activation_dropout(self, node_repr)

    def _weight_and_input(self, x):
        """The layer's [R, K, D] weight (basis-composed, zero-padded to the kernels' widths) and the input, padded to match."""
        if self.regularizer == "bdd":  # (the dense route: the blocks expanded to [R, K, D], the code below unchanged)
            weight = B.bdd_dense_weight(self.weight)
        elif self.num_bases < self.num_rels:  # basis decomposition, RGCN.py:286-301
            weight = th.matmul(self.w_comp, self.weight.view(self.num_bases, -1)).view(
                self.num_rels, self.in_feat, self.out_feat)
        else:
            weight = self.weight
        Xp = next((w for w in (32, 64, 128) if w >= self.out_feat), self.out_feat)
        if PAD_WIDTHS and x.is_cuda and Xp != self.out_feat:
            # Output widths below / between the matrix-core kernels' (the reference's RGCN experiments are 128 | 32 -> 16 | 8
            # classes, hrt/experiments/run_het_rgcn.sh): zero columns appended to the weights change no value -- the extra
            # output columns are zero and dropped, their gradients too -- and the whole layer runs on the 32 / 64 / 128-wide
            # kernels (ogbn-mag, 128 -> 8: 5.15 -> 3.9 ms per step).  HET_PAD_WIDTHS=0: the any-shape kernels as before.
            weight = nn.functional.pad(weight, (0, Xp - self.out_feat))
        Kp = _padded_in_width(self.in_feat) if x.is_cuda else self.in_feat
        if Kp != self.in_feat:  # (input widths outside 32 / 64 / 128: _padded_in_width)
            x, weight = nn.functional.pad(x, (0, Kp - self.in_feat)), nn.functional.pad(weight, (0, 0, 0, Kp - self.in_feat))
        return weight, x

    def _forward_bf16(self, g, x, norm, num_dst):
        weight, xp = self._weight_and_input(x)
        if not self.compact_as_of_node_flag:
            bias = nn.functional.pad(self.h_bias, (0, weight.shape[2] - self.out_feat)) if self.bias else None
            if B.rgcn_layer_fused_applies(g, xp, weight, norm, bias):
                # the bf16 kernels, the bias inside them: the output is rounded once; slicing rounds nothing
                node_repr = B.rgcn_layer1_separate_coo(g, xp, weight, norm, bias)
                if num_dst is not None and num_dst < node_repr.shape[0]:
                    node_repr = node_repr[:num_dst]
                if node_repr.shape[1] != self.out_feat:
                    node_repr = node_repr[:, :self.out_feat]
                return _activation_dropout(self, node_repr)
        self._upcast_of_bf16 = True  # (a bdd layer: the fp32 pass below is part of this call's dense route, not a call of its own)
        try:
            return self.forward(g, x.float(), norm, num_dst).to(th.bfloat16)
        finally:
            self._upcast_of_bf16 = False


def _heads_first(w, H):
    """[R, 1, in, H*dk] typed projection weights -> [R, H, in, dk] (head h = columns h*dk .. (h+1)*dk)."""
    R, _, K, X = w.shape
    return w.view(R, K, H, X // H).permute(0, 2, 1, 3)


class HET_HGTLayerHetero(nn.Module):
    """Heterogeneous graph transformer layer (HGT/models.py:15-286): typed K/Q/V projections per node type,
    per-relation attention and message weights, edge softmax with the relation prior as temperature, typed
    output projection gated by sigmoid(skip).

    ``multiply_among_weights_first_flag`` (HGT/models.py:124-151, in the reference's sweep hrt/utils/_do_all_cases.sh:6,34
    with --num_heads 1): the typed K / Q / V projections are folded into the per-relation weights --
    W_att[r,h] = Q_dt(r),h . att[r,h] . K_st(r),h^T ([in,in]; K . att . Q^T for the fused score op) and
    W_msg[r,h] = V_st(r),h . msg[r,h] ([in,dk]) -- and the edge ops take the layer input itself as k = q = v.  The
    reference's code for it reshapes with ``view`` where a transpose is meant, multiplies relation_msg and V in the
    opposite order and indexes V by the destination type (its own "fixme"s): taken literally it is a different model and
    only type-checks for one head with in_dim == d_k.  Built here with the INTENDED meaning -- the same function as the
    layer without the flag (associativity), any number of heads -- which is what oracle/layers.py::hgt_layer checks.

    bf16 activations: a ``torch.bfloat16`` input ``h`` gives a bf16 output, and a bf16 output gradient a bf16 ``h.grad``.  All
    parameters (k / q / v / a_linears, relation_att / msg / pri, skip), the folded per-relation weights and every parameter
    gradient stay fp32.  On the fused path the rows gathered once per edge are bf16: ``kv_c`` ([k' | m] of every (relation,
    source) row) and ``q`` are rounded once at their GEMM's store (bf16 ``h`` widened on load, fp32 weight and accumulation);
    ``new_h`` is rounded once from the fp32 ``acc / sum`` (whole destinations and hubs alike); the layer output and the gradient
    of ``new_h`` once by the typed output projection; ``h.grad`` once, after all of a node's terms are summed in the node-major
    pass.  The log-sum-exp, the gradients of ``kv_c`` and ``q`` (sums over edges that feed the fp32 parameter gradients) and
    every sum, exponential, maximum and dot product are fp32 on widened values; rounding is to nearest even.
    Which calls the bf16 kernels serve (NATIVE), and which code serves every other call, fp32 or bf16, is decided in one place: the
    table in het_amd/backend/hgt_route.py.  A bf16 call outside NATIVE (path ``upcast``) is correct, not faster: it runs fp32 on an
    upcast copy of ``h`` and the result is cast back to bf16 (the gradient likewise, through autograd).
    One form of the backward inside the bf16 path keeps an fp32 buffer (``dx`` = fp32_buffer of that table): it adds a node's
    gradient terms relation by relation in an fp32 [N, in] buffer and rounds it once; ``h``, ``kv_c``, ``q`` and ``new_h`` are bf16
    there too.

    ``use_norm`` (the HGT paper's x = norm_t(W[t] . Agg(x)); HGT/models_dgl.py:131-138 applies the per-type ``LayerNorm(out_dim)`` the
    HET class only builds, HGT/models.py:92-97): the layer's output y, on the full [N, out] result and before the ``num_dst`` slice,
    becomes (y - mean) * rsqrt(var + norm_eps) * norm_weight[t] + norm_bias[t] per row, t the row's node type, var biased --
    one HIP launch forward, two backward (backend/hgt_fused_layer.py: typed_layer_norm), at the end of every path above.
    ``norm_weight`` (ones) and ``norm_bias`` (zeros) [T, out_dim] exist only with ``use_norm``; ``self.drop`` stays unapplied, as
    in the reference's HET class.  A node without in-edges has y = 0, so its row is ``norm_bias[t]`` exactly.  Output widths that are
    no multiple of 4 (10 classes) take F.layer_norm per type: correct, not fast.  bf16 activations add two roundings to the
    contract above: on the bf16 kernels' path the norm reads the bf16 y the output projection stored, computes in fp32 and rounds
    ``out`` once at its store, and its backward rounds ``grad_y`` once (the row statistics, norm_weight / norm_bias and their
    gradients are fp32); on the upcast paths the norm runs in fp32 with the rest and the layer's one rounding follows it.  y is
    kept for the backward: N * out * sizeof(row type) more memory than without the norm."""

    def __init__(self, num_ntypes, num_rels, in_dim, out_dim, num_heads=1, dropout=0.2, use_norm=False,
                 hgt_fused_attn_score_flag=False, compact_as_of_node_flag=False, compact_direct_indexing_flag=False,
                 fused_message_mean_aggregation_flag=True, multiply_among_weights_first_flag=False):
        super().__init__()
        if not fused_message_mean_aggregation_flag:  # (the reference's HGT/models.py:251-277 branch)
            B.hgt_full_graph_edge_softmax_and_message_mean_aggregation_csr(None, None, None, None)  # raises HetUnsupported, named
        self.num_ntypes, self.num_relations, self.in_dim, self.out_dim = num_ntypes, num_rels, in_dim, out_dim
        self.num_heads, self.d_k = num_heads, out_dim // num_heads
        self.sqrt_dk = math.sqrt(self.d_k)
        self.hgt_fused_attn_score_flag = hgt_fused_attn_score_flag
        self.compact_as_of_node_flag = compact_as_of_node_flag
        self.compact_direct_indexing_flag = compact_direct_indexing_flag
        self.multiply_among_weights_first_flag = multiply_among_weights_first_flag
        self.k_linears = nn.Parameter(th.Tensor(num_ntypes, 1, in_dim, out_dim))
        self.q_linears = nn.Parameter(th.Tensor(num_ntypes, 1, in_dim, out_dim))
        self.v_linears = nn.Parameter(th.Tensor(num_ntypes, 1, in_dim, out_dim))
        self.a_linears = nn.Parameter(th.Tensor(num_ntypes, 1, out_dim, out_dim))
        self.relation_pri = nn.Parameter(th.ones(num_rels, num_heads))
        self.relation_att = nn.Parameter(th.Tensor(num_rels, num_heads, self.d_k, self.d_k))
        self.relation_msg = nn.Parameter(th.Tensor(num_rels, num_heads, self.d_k, self.d_k))
        self.skip = nn.Parameter(th.ones(num_ntypes, 1, 1, 1))
        self.drop = nn.Dropout(dropout)
        self.use_norm, self.norm_eps = bool(use_norm), 1e-5
        if self.use_norm:  # (registered only then: a layer without the norm keeps the state_dict it had)
            self.norm_weight = nn.Parameter(th.ones(num_ntypes, out_dim))
            self.norm_bias = nn.Parameter(th.zeros(num_ntypes, out_dim))
        self.reset_parameters()

    def reset_parameters(self):
        for p in (self.relation_att, self.relation_msg, self.k_linears, self.q_linears, self.v_linears, self.a_linears):
            nn.init.xavier_uniform_(p)

    def forward(self, G, h, num_dst=None):
        """``num_dst``: ``G`` is a sampled block whose first ``num_dst`` nodes are its destinations (only their rows are
        returned); its nodes are runs of equal type (``node_segment_types``, het_amd/sampling.py) instead of one run per type."""
        _refuse_inference_graph(G, self, lambda: _needs_grad(h, self))
        offs = G.get_original_node_type_offsets()
        route = self._route(G, h, offs)
        if route.path == "upcast":
            # correct, not faster: the fp32 layer on an upcast copy -- the norm of use_norm runs in fp32 with the rest -- and one
            # final rounding (class docstring); autograd casts the gradient of the input back
            return self.forward(G, h.float(), num_dst).to(th.bfloat16)
        seg_types = G.graph_data["original"].get("node_segment_types") if hasattr(G, "graph_data") else None
        per_run = (lambda w: w) if seg_types is None else (lambda w: w.index_select(0, seg_types))
        out = getattr(self, "_forward_" + route.path)(route, G, h, offs, per_run)  # _forward_fused, _weights_first, _composition
        # use_norm on the full [N, out] result (one affine pair per run of ``offs``), then the destinations' rows
        if self.use_norm:
            out = _hgt_fused.typed_layer_norm(out, offs, per_run(self.norm_weight), per_run(self.norm_bias), self.norm_eps)
        return out if num_dst is None else out[:num_dst]

    def _route(self, G, h, offs):
        """Which code serves the call: the facts hgt_route.decide reads (its Facts) and its answer."""
        graph, canonical, num_dst_rows, rels_per_type = _hgt_fused.graph_facts(G, offs)
        d_pad = _hgt_fused._padded_head(self.d_k)
        facts = hgt_route.Facts(
            cuda=h.is_cuda, bf16=h.dtype == th.bfloat16, dim=h.dim(), N=h.shape[0], K_padded=_padded_in_width(self.in_dim),
            H=self.num_heads, d_pad=d_pad, groups=_hgt_fused._head_groups(self.num_heads, d_pad), out_dim=self.out_dim,
            plan=B.plan_enabled(), fused=_hgt_fused.FUSED, weights_first_flag=self.multiply_among_weights_first_flag,
            fused_attn_score_flag=self.hgt_fused_attn_score_flag, compact_flag=self.compact_as_of_node_flag,
            direct_flag=self.compact_direct_indexing_flag, compact_dst_below=_hgt_fused.COMPACT_DST_BELOW, **graph)
        return hgt_route.decide(facts, canonical, num_dst_rows, rels_per_type)

    def _forward_fused(self, route, G, h, offs, per_run):
        """Attention + aggregation as one node on the distinct (relation, source) rows (backend/hgt_fused_layer.py): the same
        function of the parameters for every flag combination of the composition, without the per-edge tensors."""
        k_w, q_w, v_w = self.k_linears, self.q_linears, self.v_linears
        if route.Kp != self.in_dim:  # (the layer input meets the three typed projections only: zero columns / zero weight rows)
            rows = (0, 0, 0, route.Kp - self.in_dim)
            h = nn.functional.pad(h, (0, route.Kp - self.in_dim))
            k_w, q_w, v_w = nn.functional.pad(k_w, rows), nn.functional.pad(q_w, rows), nn.functional.pad(v_w, rows)
        return _hgt_fused.hgt_layer_fused(route, G, h, offs, per_run(q_w), per_run(th.sigmoid(self.skip) * self.a_linears), k_w, v_w,
                                          self.relation_att, self.relation_msg, self.relation_pri, self.num_heads,
                                          self.hgt_fused_attn_score_flag)

    def _forward_composition(self, route, G, h, offs, per_run):
        """The reference's model code op by op (HGT/models.py:120-262); ``route.score`` / ``route.direct``: the form of the score."""
        k, q, v = (B.rgnn_relational_matmul_no_scatter_gather_list(offs, per_run(w), h).view(-1, self.num_heads, self.d_k)
                   for w in (self.k_linears, self.q_linears, self.v_linears))
        return self._edge_ops(route, G, offs, per_run, self.relation_att, self.relation_msg, k, q, v, q)

    def _edge_ops(self, route, G, offs, per_run, att, msg, k, q, v, q_rows):
        """The attention score in the form of ``route.score``, the edge softmax fused with the message aggregation, and the typed
        output projection.  ``q_rows``: what the relation weights ``att`` multiply on the destination side -- q, or [N, in] rows
        with one head (--multiply_among_weights_first_flag)."""
        one_head = q_rows.dim() == 2
        # The per-edge tensor q[dst] . relation_att[r] of the default flags (models.py:215-241) is read by the inner
        # product only and its rows repeat for every edge of a (relation, destination) pair: when the graph carries the
        # unique (relation, node) lists it is formed on those rows and indexed directly -- the reference's compact
        # dataflow, same values -- instead of being written and re-read as an [E,H,dk] tensor.
        if route.score == "fused_score":  # models.py:172-175
            attn_score = B.hgt_full_graph_hetero_attention_ops_coo(G, att, k, q)
        elif route.score == "compact":  # models.py:177-214
            ss = G.get_separate_unique_node_indices_single_sided()
            compact = B.rgnn_relational_matmul(
                {"unique_srcs_and_dests_rel_ptrs": ss["rel_ptrs_col"],
                 "unique_srcs_and_dests_node_indices": ss["node_indices_col"]}, att, q_rows, one_head, 1)
            attn_score = B.rgnn_inner_product_right_node(G, compact, k, 2 if route.direct else 1, "_col")
        else:  # models.py:215-241
            s = G.get_separate_coo_original()
            per_edge = B.rgnn_relational_matmul(
                {"separate_coo_rel_ptrs": s["rel_ptrs"], "separate_coo_node_indices": s["col_indices"],
                 "separate_coo_eids": s["eids"]}, att, q_rows, one_head, 0)
            attn_score = B.rgnn_inner_product_right_node(G, per_edge, k, 0, "_col")
        new_h = B.hgt_full_graph_message_calc_edge_softmax_and_message_mean_aggregation_coo(
            msg, v, G, (self.relation_pri / self.sqrt_dk), attn_score)
        return B.rgnn_relational_matmul_no_scatter_gather_list(
            offs, per_run(th.sigmoid(self.skip) * self.a_linears), new_h.view(-1, self.out_dim))

    def _forward_weights_first(self, route, G, h, offs, per_run):
        """--multiply_among_weights_first_flag (see the class docstring): two small batched products per step replace the three
        typed projections of the nodes; the per-relation [in,in] / [in,dk] weights then meet the layer input directly."""
        H, dk = self.num_heads, self.d_k
        st, dt = G.get_rel_node_types()
        Kr = _heads_first(self.k_linears.index_select(0, st), H)  # [R,H,in,dk]
        Qr = _heads_first(self.q_linears.index_select(0, dt), H)
        Vr = _heads_first(self.v_linears.index_select(0, st), H)
        if self.hgt_fused_attn_score_flag:  # s = < k[src] . att, q[dst] > = h[src] . (K att Q^T) . h[dst]^T
            w_att = th.matmul(th.matmul(Kr, self.relation_att), Qr.transpose(2, 3))
        else:                               # s = < q[dst] . att, k[src] > = h[dst] . (Q att K^T) . h[src]^T
            w_att = th.matmul(th.matmul(Qr, self.relation_att), Kr.transpose(2, 3))
        w_msg = th.matmul(Vr, self.relation_msg)  # [R,H,in,dk]
        hh = h.unsqueeze(1) if H == 1 else h.unsqueeze(1).expand(-1, H, -1)
        hh = hh.contiguous()  # k = q = v: the layer input once per head (the reference: h.unsqueeze(1).repeat(1, H, 1))
        # (per edge: [E,H,in] = h[dst] . W_att[r,h], from the one-head rows of h)
        return self._edge_ops(route, G, offs, per_run, w_att.contiguous(), w_msg.contiguous(), hh, hh, hh, h)
