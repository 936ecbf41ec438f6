"""MF — drop-in for reference models/mf.py: two embedding Linears and a row-wise dot product (mf.py:28-32)."""
import torch
from torch import nn

from ... import native
from ..util import require_gpu, row_major_embedding_, use_native
from .base import NCF
from .basic_ncf import _ScoringMixin


class MF(_ScoringMixin, NCF):
    compatible_datasets = ("FixedPointwiseDataset", "FixedRankingDataset")

    def __init__(self, item_dim, user_dim, item_emb=128, user_emb=128):
        super().__init__()
        self.kwargs = {'item_dim': item_dim, 'user_dim': user_dim, 'item_emb': item_emb, 'user_emb': user_emb}
        self.item_embeddings = nn.Sequential(row_major_embedding_(nn.Linear(item_dim, item_emb)))
        self.user_embeddings = nn.Sequential(row_major_embedding_(nn.Linear(user_dim, user_emb)))

    def get_model_parameters(self) -> dict:
        return self.kwargs

    @property
    def num_users(self) -> int:
        return self.user_embeddings[0].in_features

    @property
    def num_items(self) -> int:
        return self.item_embeddings[0].in_features

    def forward(self, X_user, X_item):
        indexed = X_user.dtype == torch.int64 and X_user.dim() == 1
        if not use_native(self):
            if indexed:
                ue, ie = self.user_embeddings[0], self.item_embeddings[0]
                if (self.training and X_user.is_cuda and getattr(ue.weight, "_ncf_row_grads", None) is not None
                        and getattr(ie.weight, "_ncf_row_grads", None) is not None):
                    # both weights marked by optim.RowSparseAdam: the HIP gather, whose backward hands the optimiser
                    # (ids, gradient rows) instead of building two dense table gradients
                    from ...autograd import GatherColumnsFn
                    u = GatherColumnsFn.apply(ue.weight, ue.bias, X_user.contiguous())
                    i = GatherColumnsFn.apply(ie.weight, ie.bias, X_item.contiguous())
                else:
                    u, i = ue.weight.t()[X_user] + ue.bias, ie.weight.t()[X_item] + ie.bias
            else:
                u, i = self.user_embeddings(X_user), self.item_embeddings(X_item)
            return torch.bmm(u.unsqueeze(1), i.unsqueeze(2)).view(-1, 1)
        require_gpu(X_user, X_item)
        cache = self._refresh()  # one parameter fingerprint per forward
        if indexed:
            return native.gather_dot(self._table("user", self.user_embeddings[0], cache), X_user.contiguous(),
                                     self._table("item", self.item_embeddings[0], cache), X_item.contiguous())
        ue, ie = self.user_embeddings[0], self.item_embeddings[0]
        u = native.linear(X_user.float().contiguous(), self._dense_weight("user", ue, cache), ue.bias.detach())
        i = native.linear(X_item.float().contiguous(), self._dense_weight("item", ie, cache), ie.bias.detach())
        return native.gather_dot(u, None, i, None, B=u.shape[0])

    def softmax_loss(self, users, items, scale: float = 1.0):
        """Per-row softmax cross-entropy of each positive (users[b], items[b]) over the WHOLE catalogue:
        ``logsumexp_j(scale * <u_b, q_j>) - scale * <u_b, q_items[b]>``, (B,) fp32, with autograd — ``DotSoftmaxLossFn``, which never
        builds the B x num_items logits.  The tables are the embedding Linears on one-hot ids, ``weight.t() + bias``.  When both
        weights are marked by optim.RowSparseAdam the user rows come from GatherColumnsFn, whose backward hands (ids, gradient
        rows) to the optimiser; the item table's gradient is dense either way (every item is in every denominator)."""
        from ...autograd import DotSoftmaxLossFn, GatherColumnsFn
        require_gpu(users, items)
        ue, ie = self.user_embeddings[0], self.item_embeddings[0]
        users, items = users.long().contiguous(), items.long().contiguous()
        item_table = ie.weight.t() + ie.bias
        if getattr(ue.weight, "_ncf_row_grads", None) is not None and getattr(ie.weight, "_ncf_row_grads", None) is not None:
            return DotSoftmaxLossFn.apply(GatherColumnsFn.apply(ue.weight, ue.bias, users), item_table, None, items, scale)
        return DotSoftmaxLossFn.apply(ue.weight.t() + ue.bias, item_table, users, items, scale)
