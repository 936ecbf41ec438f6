"""Fused Adam on the HIP path: ``torch.optim.Adam``'s update (the optimiser of the reference's train.py:55) as ONE kernel
per parameter tensor (libncf_hip.so ``ncf_adam_step``) instead of torch's ~9 foreach kernels.  At BASELINE config 2 the
dense Adam over the 71 M embedding parameters is the largest part of a training step (the Linear-layout embeddings make
every gradient dense, and Adam moves every moment every step even where the gradient is zero).  ``RowSparseAdam`` is the
opt-in answer to that: the id-major embedding weights receive per-occurrence gradient ROWS instead of dense gradients and
only the rows a batch touched are updated (``ncf_adam_rows``)."""
from __future__ import annotations

import torch

from . import native
from .neural_collaborative_filtering.util import is_row_major_embedding


class FusedAdam(torch.optim.Optimizer):
    """Drop-in for ``torch.optim.Adam(params, lr, betas, eps, weight_decay)`` (amsgrad / maximize / capturable are
    not supported) on fp32 CUDA parameters; any other parameter raises (there is no CPU path in this package)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        if lr < 0 or eps < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1 or weight_decay < 0:
            raise ValueError("invalid Adam hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda or p.dtype != torch.float32 or p.grad.is_sparse:
                    raise RuntimeError("FusedAdam needs dense fp32 parameters on the GPU")
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p)          # preserve_format: the parameter's own strides
                    st["exp_avg_sq"] = torch.zeros_like(p)
                st["step"] += 1
                m, v, g = st["exp_avg"], st["exp_avg_sq"], p.grad
                # the update is elementwise: any layout works as long as all four tensors share it.  Embedding weights are
                # stored id-major (transpose views, util.row_major_embedding_): run on the contiguous transposes.
                if p.dim() == 2 and not p.is_contiguous() and p.t().is_contiguous():
                    pv, mv, vv = p.t(), m.t(), v.t()
                    gv = g.t() if g.t().is_contiguous() else g.t().contiguous()
                elif p.is_contiguous():
                    pv, mv, vv = p, m, v
                    gv = g if g.is_contiguous() else g.contiguous()
                else:
                    raise RuntimeError("FusedAdam needs contiguous (or transposed-contiguous) parameters")
                native.adam_step_(pv, gv, mv, vv, group["lr"], b1, b2, group["eps"], group["weight_decay"], st["step"])
                # the kernel writes through raw pointers: tell autograd / the models' derived-tensor caches (tables, packed
                # MLP blobs, propagated graph tables are keyed on (data_ptr, _version)) that the parameter changed
                torch.autograd.graph.increment_version(p)
        return loss


class RowSparseAdam(FusedAdam):
    """``FusedAdam`` whose id-major embedding weights (``util.row_major_embedding_``: what BasicNCF / MF construct) are updated
    row-sparsely: only the rows a batch touched, by one deterministic kernel (``native.adam_rows_``), with no table-sized
    gradient buffer.  Every other parameter takes FusedAdam's dense update.

    ``row_sparse=None`` marks every given parameter that is id-major; a list marks exactly those (one that is not id-major,
    or is not among ``params``, raises ValueError).  A marked parameter carries a list attribute ``_ncf_row_grads``: the
    backward of ``autograd.GatherColumnsFn`` / ``GatherColumnsConcatFn`` appends ``(ids, gradient rows)`` to it and leaves
    ``.grad`` None (an indexed training forward of BasicNCF, and of MF when both its weights are marked).  ``step()`` then, per
    marked parameter:
      * pending rows, no ``.grad``: the pending entries are concatenated (BPR's two forwards give two per table) and rows
        ``ids`` of the weight and of both moments take one Adam update each with the sum of their gradient rows;
      * a dense ``.grad``, nothing pending (the dense-feature ``LinearFn`` route): the inherited dense update;
      * both: RuntimeError (checked for every parameter before anything is updated);
      * neither: skipped, but its ``step`` count advances (the count is per tensor, as torch.optim.SparseAdam's).

    What differs from dense Adam — the semantics of torch.optim.SparseAdam: a row no batch touched is not moved, so weight
    decay and the decay of both moments are LAZY (they act on a row only in the steps that touch it), while the bias
    corrections use the tensor-wide step count.  When every row is touched in every step the update equals FusedAdam's.
    ``torch.nn.utils.clip_grad_norm_`` does NOT see row gradients (a marked weight's ``.grad`` is None).

    The state (``step``, ``exp_avg``, ``exp_avg_sq``, in the parameter's own layout) is FusedAdam's: a ``state_dict()`` moves
    between the two.  ``zero_grad()`` also drops pending rows; ``close()`` removes the marks, after which a backward produces
    dense gradients again.  All parameters must be fp32 CUDA tensors when the optimiser is built (move the model first)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, row_sparse=None):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        mine = [p for group in self.param_groups for p in group["params"]]
        if row_sparse is None:
            marked = [p for p in mine if is_row_major_embedding(p)]
        else:
            marked = list(row_sparse)
            for p in marked:
                if not is_row_major_embedding(p):
                    raise ValueError("row_sparse: not an id-major embedding weight (util.row_major_embedding_)")
                if not any(p is q for q in mine):
                    raise ValueError("row_sparse: a parameter this optimiser was not given")
        for p in mine:
            if not p.is_cuda or p.dtype != torch.float32:
                raise RuntimeError("RowSparseAdam needs fp32 parameters on the GPU (there is no CPU path in this package)")
        self._row_sparse = marked
        for p in marked:
            p._ncf_row_grads = []

    def _marked(self):
        return [(group, p) for group in self.param_groups for p in group["params"] if getattr(p, "_ncf_row_grads", None) is not None
                and any(p is q for q in self._row_sparse)]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        marked = self._marked()
        for _, p in marked:
            if p._ncf_row_grads and p.grad is not None:
                raise RuntimeError("RowSparseAdam: a row-sparse parameter has both a dense .grad and pending row gradients")
        for group, p in marked:
            if p.grad is not None:
                continue                                     # dense route: the inherited update below
            st = self.state[p]
            if not st:
                st["step"] = 0
                st["exp_avg"] = torch.zeros_like(p)          # preserve_format: id-major like the parameter
                st["exp_avg_sq"] = torch.zeros_like(p)
            st["step"] += 1
            pending = p._ncf_row_grads
            if not pending:
                continue
            if len(pending) == 1:
                ids, g = pending[0]                          # the column half of dX as it is: no copy
            else:
                ids, g = torch.cat([e[0] for e in pending]), torch.cat([e[1] for e in pending])
            b1, b2 = group["betas"]
            native.adam_rows_(p.t(), st["exp_avg"].t(), st["exp_avg_sq"].t(), ids, g, group["lr"], b1, b2, group["eps"],
                              group["weight_decay"], st["step"])
            torch.autograd.graph.increment_version(p)        # raw-pointer write: see FusedAdam.step
            pending.clear()
        super().step()
        return loss

    def zero_grad(self, set_to_none: bool = True):
        super().zero_grad(set_to_none=set_to_none)
        for p in self._row_sparse:
            pending = getattr(p, "_ncf_row_grads", None)
            if pending is not None:
                pending.clear()

    def close(self):
        """Remove the marks: the autograd blocks build dense gradients again and step() is FusedAdam's."""
        for p in self._row_sparse:
            if hasattr(p, "_ncf_row_grads"):
                del p._ncf_row_grads
        self._row_sparse = []
