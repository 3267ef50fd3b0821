"""Optimizers for the row-sparse gradients of ``HET_RelGraphEmbed(sparse=True)`` (het_amd/layers.py).

    embed = HET_RelGraphEmbed(N, K, sparse=True).cuda()
    opt = RowSparseAdam(embed.parameters(), lr=0.01)
    rows = embed(block.nodes)            # [B, K]; the gradient of embed.embeds is a sparse [N, K] tensor of B rows
    ...
    loss.backward(); opt.step(); opt.zero_grad()
"""
from __future__ import annotations

import math

import torch

from . import kernels as _k


class RowSparseAdam(torch.optim.Optimizer):
    """Lazy Adam for sparse gradients: ``torch.optim.SparseAdam``'s rule as one HIP launch per parameter (csrc/rows_embed.hip).

    For every row r that the gradient names, with g the sum of the gradient's entries for r:

        exp_avg[r]    = beta1 * exp_avg[r]    + (1 - beta1) * g
        exp_avg_sq[r] = beta2 * exp_avg_sq[r] + (1 - beta2) * g * g
        p[r]         -= lr * sqrt(1 - beta2^step) / (1 - beta1^step) * exp_avg[r] / (sqrt(exp_avg_sq[r]) + eps)

    Rows the gradient does not name keep p, exp_avg and exp_avg_sq bit for bit while ``step`` advances: their moments do not decay
    -- a different optimizer from dense Adam, not an approximation of it.  eps is added to sqrt(exp_avg_sq) before the bias
    correction, as SparseAdam does (dense Adam adds it to sqrt(exp_avg_sq / (1 - beta2^step))).

    The state names are SparseAdam's (``step``, ``exp_avg``, ``exp_avg_sq``), so a state_dict moves between the two.  A parameter whose
    ``.grad`` is None is skipped; a dense ``.grad`` raises with SparseAdam's message.  A sparse gradient has one sparse dimension (row
    ids) over dense rows, as ``nn.Embedding(sparse=True)`` and ``HET_RelGraphEmbed(sparse=True)`` give.  A coalesced gradient goes to
    the kernel as it is; an uncoalesced one costs one stable sort of its B ids, and the kernel sums the rows of equal ids in their
    original order (no atomics: the same bits every run).

    A contiguous float32 GPU parameter [N, K] with K a multiple of 4 up to 1024 takes the kernel; CPU parameters and other shapes the
    same rule composed from torch ops.

    Not supported: weight decay, amsgrad, maximize, and parameters sharded or replicated over several processes (het_amd/dist.py):
    nothing here reduces a sparse gradient across ranks."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        if not 0.0 < lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 < eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        super().__init__(params, {"lr": lr, "betas": betas, "eps": eps})
        for group in self.param_groups:
            for p in group["params"]:
                if p.is_sparse or p.is_complex():
                    raise ValueError("RowSparseAdam requires dense, real parameter tensors")

    @staticmethod
    def _kernel_ok(p, m, v, vals) -> bool:
        return (p.is_cuda and p.dim() == 2 and _k.rows_embed_ok(p.shape[1])
                and all(t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0 and t.device == p.device
                        for t in (p, m, v, vals)))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            lr, (beta1, beta2), eps = group["lr"], group["betas"], group["eps"]
            if group.get("maximize", False):  # (a param group loaded from a SparseAdam state_dict may carry the key)
                raise RuntimeError("RowSparseAdam does not support maximize")
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = p.grad
                if not g.is_sparse:
                    raise RuntimeError("SparseAdam does not support dense gradients, please consider Adam instead")
                if g.sparse_dim() != 1 or g.shape != p.shape:
                    raise RuntimeError(f"RowSparseAdam: a gradient with one sparse dimension (row ids) of the parameter's shape expected, "
                                       f"got sparse_dim {g.sparse_dim()}, shape {tuple(g.shape)} for {tuple(p.shape)}")
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = 0
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state["step"] += 1
                step, m, v = state["step"], state["exp_avg"], state["exp_avg_sq"]
                if g._nnz() == 0:
                    continue
                coalesced = g.is_coalesced()
                rows, vals = g._indices()[0], g._values()
                if self._kernel_ok(p, m, v, vals):
                    perm = None
                    if not coalesced:
                        rows, perm = torch.sort(rows, stable=True)
                    _k.rows_adam_(p, m, v, rows.contiguous(), perm, vals, lr, beta1, beta2, eps, step)
                    torch.autograd.graph.increment_version(p)  # (written through a raw pointer: whatever saved the table sees it)
                    continue
                if not coalesced:
                    g = g.coalesce()
                    rows, vals = g._indices()[0], g._values()
                vals = vals.to(p.dtype)
                mr = m.index_select(0, rows).mul_(beta1).add_(vals, alpha=1 - beta1)
                vr = v.index_select(0, rows).mul_(beta2).addcmul_(vals, vals, value=1 - beta2)
                m.index_copy_(0, rows, mr)
                v.index_copy_(0, rows, vr)
                step_size = lr * math.sqrt(1 - beta2 ** step) / (1 - beta1 ** step)
                p.index_add_(0, rows, mr.div_(vr.sqrt_().add_(eps)), alpha=-step_size)
        return loss
