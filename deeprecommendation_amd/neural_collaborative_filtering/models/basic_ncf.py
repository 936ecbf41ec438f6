"""BasicNCF — drop-in for reference models/basic_ncf.py (same ctor kwargs, state_dict keys, forward signature).

forward(X_user, X_item) dispatches on the input:
  * int64 (B,) positions  -> table path: T = W^T + b per side (the reference's Linear over a one-hot row,
    basic_ncf.py:38-39 with src/util.py:5-10), gathered and scored by ONE fused HIP kernel (ncf_score_fused);
  * float (B, dim) rows   -> dense path: the two Linears as HIP GEMMs, then the same fused MLP kernel on the
    (B, E) activations (identity gather).
With content attached (``set_content``: the reference's FixedProfilesProvider form, item_dim = user_dim = F) int64 positions name
rows of the content tables and the table path runs on T = content·W^T + b, built once per weight version.
Both run only on CUDA(HIP) tensors in eval / no-grad mode; a training step uses the differentiable torch ops.
"""
import torch
from torch import nn

from ... import native
from ..util import (build_MLP_layers, is_row_major_embedding, mlp_linears, params_version, require_gpu, row_major_embedding_,
                    use_native)
from .base import NCF


class _ScoringMixin:
    """Derived inference tensors shared by BasicNCF / MF / GraphNCF: embedding tables and packed MLP weights."""

    scoring_dtype = torch.float32
    fold_first_layer = False
    partial_first_layer = None      # None = automatic (see _partial), True = whenever supported, False = never
    partial_max_bytes = None        # cap on the partial table; None = min(4 GiB, free device memory / 4) at build time
    PARTIAL_MIN_ROUNDS = 1          # automatic mode: batches of at least this many rounds of 4 x CUs 32-pair tiles
    _content = None                 # BasicNCF.set_content: (user_profiles (U, user_dim), item_features (I, item_dim)); None = one-hot form

    def set_partial_first_layer(self, enabled=None, max_bytes=None):
        """Partial first layer (frozen weights, bit-identical): layer 1's accumulators after the user table's k-groups are
        stored once per weight version for every row of that table (native.layer1_partial) and each pair's layer 1 starts
        from them (native.score_fused_partial): 3/4 of the MFMAs per pair at 128-256-128-1.  ``None`` (default) = automatic:
        fp32 table scoring of a large enough batch, from the second forward of a weight version on, never built inside a
        stream capture, and only while the table fits ``max_bytes``.  ``True`` = whenever supported, ``False`` = never."""
        self.partial_first_layer = None if enabled is None else bool(enabled)
        self.partial_max_bytes = max_bytes
        self._native_ver = None
        return self

    def set_fold_first_layer(self, enabled: bool = True):
        """Opt-in inference-time folding (frozen weights): relu(W1·cat(a, b) + b1) == relu(PA[ia] + PB[ib]) with
        PA = TA·W1[:, :EA]^T + b1 and PB = TB·W1[:, EA:]^T built once per weight version.  The first MLP layer then
        costs no matrix work per pair (ncf_score_folded); the tables grow from E to N1 floats per row.  Same function
        up to fp32 summation order.  Applies to fp32 MLPs with two hidden layers that have a kernel instance."""
        self.fold_first_layer = bool(enabled)
        self._native_ver = None
        return self

    def set_scoring_dtype(self, dtype):
        """float32 (default; 1e-5 parity with the reference) or bfloat16 (BASELINE config 5: bf16 tables and MLP
        weights, fp32 accumulate and output).  Only the int64-position table path has a bf16 kernel."""
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("scoring dtype must be float32 or bfloat16")
        self.scoring_dtype = dtype
        self._native_ver = None
        return self

    def _refresh(self):
        ver = params_version(self)
        if getattr(self, "_native_ver", None) != ver:
            self._native_cache = {}
            self._native_ver = ver
        return self._native_cache

    # Every helper below takes the dict returned by ONE `_refresh()` per forward: the parameter fingerprint walks the
    # module tree (≈ 12 µs on the host) and a forward used to pay it three times (49 µs per call, measured).
    def _table(self, name: str, lin: nn.Linear, cache=None) -> torch.Tensor:
        cache = self._refresh() if cache is None else cache
        if name not in cache:
            with torch.no_grad():
                if self._content is not None:
                    # content form (BasicNCF.set_content): row i = content[i] . W^T + b, the Linear of the float-row forward over
                    # every content row, once per weight version
                    content = self._content[0 if name == "user" else 1]
                    emb = native.linear(content, self._dense_weight(name, lin, cache), lin.bias.detach())
                else:
                    # row i = W[:, i] + b : exactly what Linear(onehot(i)) computes (one fp32 rounding)
                    emb = lin.weight.detach().t().contiguous() + lin.bias.detach()
                cache[name] = emb.to(self.scoring_dtype).contiguous()
        return cache[name]

    def _dense_weight(self, name: str, lin: nn.Linear, cache=None) -> torch.Tensor:
        """Row-contiguous [E, num_ids] copy of an embedding weight for the dense-profile GEMM (the parameter itself is
        stored id-major, util.row_major_embedding_); cached per weight version."""
        cache = self._refresh() if cache is None else cache
        key = "dense_w::" + name
        if key not in cache:
            cache[key] = lin.weight.detach().contiguous()
        return cache[key]

    def _packed_mlp(self, name: str = "MLP", cache=None):
        cache = self._refresh() if cache is None else cache
        key = "packed::" + name
        if key not in cache:
            lins = mlp_linears(getattr(self, name))
            try:
                cache[key] = native.PackedMLP([l.weight for l in lins], [l.bias for l in lins], dtype=self.scoring_dtype)
            except native.NativeError as e:
                if e.code != native.NCF_EUNSUPPORTED:
                    raise
                cache[key] = None
        return cache[key]

    def _folded(self, tabA, tabB, mlp_name, cache=None):
        """(PA, PB, packed tail MLP) for the folded path, cached per weight version and table pair; None if the MLP
        shape has no folded kernel."""
        cache = self._refresh() if cache is None else cache
        key = ("folded", mlp_name, tabA.data_ptr(), tabB.data_ptr(), tuple(tabA.shape), tuple(tabB.shape))
        if key not in cache:
            lins = mlp_linears(getattr(self, mlp_name))
            ok = (len(lins) == 3 and lins[2].out_features == 1 and lins[0].in_features == tabA.shape[1] + tabB.shape[1]
                  and native.folded_supported(lins[0].out_features, lins[1].out_features))
            if not ok:
                cache[key] = None
            else:
                EA = tabA.shape[1]
                w1 = lins[0].weight.detach()
                PA = native.linear(tabA, w1[:, :EA].contiguous(), lins[0].bias.detach())       # b1 folded into PA
                PB = native.linear(tabB, w1[:, EA:].contiguous(), None)
                tail = native.PackedMLP([lins[1].weight, lins[2].weight], [lins[1].bias, lins[2].bias])
                cache[key] = (PA, PB, tail, tabA, tabB)  # keep the source tables alive: the key holds their addresses
        hit = cache[key]
        return None if hit is None else hit[:3]

    def _partial(self, tabA, idxA, tabB, packed, mlp_name, cache):
        """The partial-first-layer table P for (tabA, packed), or None when this forward takes native.score_fused.  P and
        the count of forwards that could have used it live in the _refresh() cache, so the next weight version drops them.
        Only a table that this cache owns qualifies (P is keyed on its address; a per-forward tensor's address is reused
        by the caching allocator)."""
        mode = self.partial_first_layer
        if mode is False or self.fold_first_layer or idxA is None or tabB is None or tabA.dtype != torch.float32:
            return None
        key = ("partial", mlp_name, tabA.data_ptr())
        ent = cache.get(key)
        if ent is None:
            owned = any(v is tabA or (isinstance(v, tuple) and any(x is tabA for x in v)) for v in cache.values())
            ok = owned and native.partial_supported(tabA.shape[1], tabB.shape[1], packed)
            ent = cache[key] = {"ok": ok, "seen": 0, "P": None}
        if not ent["ok"]:
            return None
        P = ent["P"]
        if P is None:
            ent["seen"] += 1
            if mode is None:
                dev = tabA.device
                round_pairs = 4 * 32 * torch.cuda.get_device_properties(dev).multi_processor_count
                if ent["seen"] < 2 or idxA.numel() < self.PARTIAL_MIN_ROUNDS * round_pairs:
                    return None
            if torch.cuda.is_current_stream_capturing():
                return None
            nbytes = (tabA.shape[0] + 1) * packed.dims[1] * 4
            cap = self.partial_max_bytes
            if cap is None:
                cap = min(4 << 30, torch.cuda.mem_get_info(tabA.device)[0] // 4)
            if nbytes > cap:
                return None
            try:
                P = ent["P"] = native.layer1_partial(tabA, packed)
            except native.NativeError as e:
                if e.code != native.NCF_EUNSUPPORTED:
                    raise
                ent["ok"] = False
                return None
        return P

    def _score(self, tabA, idxA, tabB, idxB, mlp_name="MLP", cache=None):
        """gather(A) ‖ gather(B) -> MLP -> (B,1): fused kernel when the shape has an instance, else K1 + K2."""
        EA = tabA.shape[1]
        EB = 0 if tabB is None else tabB.shape[1]
        if self.fold_first_layer and tabB is not None and tabA.dtype == torch.float32:
            folded = self._folded(tabA, tabB, mlp_name, cache)
            if folded is not None:
                PA, PB, tail = folded
                return native.score_folded(PA, idxA, PB, idxB, tail)
        cache = self._refresh() if cache is None else cache
        packed = self._packed_mlp(mlp_name, cache)
        if packed is not None and tabA.dtype == packed.dtype and packed.supports(EA, EB):
            P = self._partial(tabA, idxA, tabB, packed, mlp_name, cache)
            if P is not None:
                return native.score_fused_partial(P, tabA, idxA, tabB, idxB, packed)
            return native.score_fused(tabA, idxA, tabB, idxB, packed)
        if tabA.dtype != torch.float32:
            raise native.NativeError(native.NCF_EUNSUPPORTED, f"no bf16 kernel for EA={EA} EB={EB} MLP {getattr(packed, 'dims', None)}")
        x = native.gather_concat(tabA, idxA, tabB, idxB)
        lins = mlp_linears(getattr(self, mlp_name))
        return native.mlp_forward(x, [l.weight.detach() for l in lins], [l.bias.detach() for l in lins])


class BasicNCF(_ScoringMixin, NCF):
    compatible_datasets = ("FixedPointwiseDataset", "FixedRankingDataset")

    def __init__(self, item_dim, user_dim, dropout_rate=0.2, item_emb=256, user_emb=256, mlp_dense_layers=None):
        super().__init__()
        if mlp_dense_layers is None:
            mlp_dense_layers = [256, 128]
        self.kwargs = {'item_dim': item_dim, 'user_dim': user_dim, 'item_emb': item_emb, 'user_emb': user_emb,
                       'mlp_dense_layers': mlp_dense_layers, 'dropout_rate': dropout_rate}
        self.item_embeddings = nn.Sequential(row_major_embedding_(nn.Linear(item_dim, item_emb)))
        self.user_embeddings = nn.Sequential(row_major_embedding_(nn.Linear(user_dim, user_emb)))
        self.MLP = build_MLP_layers(item_emb + user_emb, mlp_dense_layers, dropout_rate=dropout_rate)

    def get_model_parameters(self) -> dict:
        return self.kwargs

    def set_content(self, user_profiles=None, item_features=None):
        """Content form (the reference's FixedProfilesProvider: a user is a fixed profile row, an item its feature row): attach
        the two fp32 device tables, ``user_profiles`` (U, user_dim) and ``item_features`` (I, item_dim).  int64 arguments of
        ``forward`` are then ROWS of these tables: in eval mode the embedding tables are ``content . W^T + b``, built once per
        weight version and per ``set_content``, and every table kernel (fused, partial, folded, bf16, top-K, ranks) runs on them
        as it does for a one-hot model; a training step gathers the content rows and runs the Linear of the float-row forward.
        ``set_content(None, None)`` detaches them.  Float-row forwards are not affected.  Neither table is copied or saved."""
        if user_profiles is None and item_features is None:
            self._content = None
            self._native_ver = None
            return self
        for t, what, width in ((user_profiles, "user_profiles", self.kwargs["user_dim"]), (item_features, "item_features", self.kwargs["item_dim"])):
            if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 2:
                raise ValueError(f"{what} must be a 2-D float32 tensor")
            if t.shape[1] != width:
                raise ValueError(f"{what} has {t.shape[1]} columns, the model's embedding takes {width}")
            if not t.is_contiguous():
                raise ValueError(f"{what} must be row-contiguous")
            if not t.is_cuda:
                raise ValueError(f"{what} must live on the GPU (got {t.device})")
        self._content = (user_profiles, item_features)
        self._native_ver = None
        return self

    @property
    def num_users(self) -> int:
        """Rows a user position may name: the content table's with content attached, the one-hot width otherwise."""
        return self._content[0].shape[0] if self._content is not None else self.user_embeddings[0].in_features

    @property
    def num_items(self) -> int:
        return self._content[1].shape[0] if self._content is not None else self.item_embeddings[0].in_features

    def forward(self, X_user, X_item):
        indexed = X_user.dtype == torch.int64 and X_user.dim() == 1
        if not use_native(self):
            return self._forward_train(X_user, X_item, indexed)
        require_gpu(X_user, X_item)
        cache = self._refresh()
        if indexed:
            return self._score(self._table("user", self.user_embeddings[0], cache), X_user.contiguous(),
                               self._table("item", self.item_embeddings[0], cache), X_item.contiguous(), cache=cache)
        ue, ie = self.user_embeddings[0], self.item_embeddings[0]
        u = native.linear(X_user.float().contiguous(), self._dense_weight("user", ue, cache), ue.bias.detach())
        i = native.linear(X_item.float().contiguous(), self._dense_weight("item", ie, cache), ie.bias.detach())
        return self._score(u, None, i, None, cache=cache)  # cat(user, item): basic_ncf.py:40

    def _forward_train(self, X_user, X_item, indexed):
        """Training step (dropout active, autograd recording).  On CUDA tensors the gather and the Linear(+ReLU) layers run
        forward AND backward on the HIP kernels through deeprecommendation_amd.autograd; on CPU it is plain torch."""
        if X_user.is_cuda and not getattr(self, "train_with_torch_ops", False):
            from ...autograd import GatherColumnsConcatFn, GatherColumnsFn, LinearFn, mlp_train
            ue, ie = self.user_embeddings[0], self.item_embeddings[0]
            if indexed and self._content is not None:
                # content form: the batch's (B, F) content rows, gathered by position, then the float-row step below on them
                X_user = native.gather_concat(self._content[0], X_user.contiguous())
                X_item = native.gather_concat(self._content[1], X_item.contiguous())
                indexed = False
            if indexed:
                # The parameters live in nn.Linear layout [E, U] (checkpoint compatibility), so a training step gathers
                # COLUMNS of W (materialising T = W^T + b every step for the row-gather kernel costs two full-table
                # passes: 13.6 ms per step at 1 M users).  GatherColumnsFn reads the B columns and, backward, scatters the
                # gradient straight into a zeroed [E, U] tensor; torch's `W.t()[idx]` backward sorts the ids and makes two
                # table-sized copies on the way (1.3 ms of a 3.9 ms step).
                if is_row_major_embedding(ue.weight) and is_row_major_embedding(ie.weight):
                    # both embeddings + the concat as one gather; gradient rows scattered from the halves of dX
                    x = GatherColumnsConcatFn.apply(ue.weight, ue.bias, X_user.contiguous(), ie.weight, ie.bias, X_item.contiguous())
                else:
                    x = torch.cat((GatherColumnsFn.apply(ue.weight, ue.bias, X_user.contiguous()),
                                   GatherColumnsFn.apply(ie.weight, ie.bias, X_item.contiguous())), dim=1)
            else:
                x = torch.cat((LinearFn.apply(X_user.float(), ue.weight, ue.bias, False),
                               LinearFn.apply(X_item.float(), ie.weight, ie.bias, False)), dim=1)
            return mlp_train(self.MLP, x)
        if indexed and self._content is not None:
            X_user, X_item, indexed = self._content[0][X_user], self._content[1][X_item], False
        if indexed:
            ue, ie = self.user_embeddings[0], self.item_embeddings[0]
            user_emb = ue.weight.t()[X_user] + ue.bias
            item_emb = ie.weight.t()[X_item] + ie.bias
        else:
            user_emb = self.user_embeddings(X_user)
            item_emb = self.item_embeddings(X_item)
        return self.MLP(torch.cat((user_emb, item_emb), dim=1))
