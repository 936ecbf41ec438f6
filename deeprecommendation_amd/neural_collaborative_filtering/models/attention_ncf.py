"""AttentionNCF — drop-in for reference models/attention_ncf.py:64-224 (same kwargs, state_dict keys, forward).

HIP scoring path (eval / no-grad), all arithmetic in libncf_hip.so:
  1. ItemEmbeddings on candidates and rated items                         (attention_ncf.py:150-151)  ncf_mlp_forward
  2. AttentionNet's first Linear is split at the concat boundary of :176,  W0 = [Wc | Wr]:
        pc = cand_emb @ Wc^T + b0   (B, A),   pr = rated_emb @ Wr^T   (I, A)
     so the score of a pair is  b1 + w1 . relu(pc[b] + pr[i])  — no (B·nnz, 2·IE) pair matrix, no per-pair GEMM.
  3. scores -> masked softmax -> x ratings -> weighted sum              (:182-213)                  ncf_attn_forward
     over the CSR of `user_matrix != 0` (:158).  The weighted sum uses the linearity of UserEmbeddings (:216):
        UserEmbeddings(sum_i a_i f_i) = sum_i a_i (f_i @ Wu^T) + bu
     so the kernel aggregates the projected rows P = rated_items @ Wu^T (I, UE) instead of F-wide feature rows.
  4. cat(candidate_emb, user_emb) -> MLP                                 (:219-222)                  ncf_score_fused
Both reformulations change only the fp32 summation order (tests hold them to 1e-5 relative of the reference).
A training step keeps to differentiable torch ops with the reference's train-only message dropout and target mask.
"""
import sys

import torch
import torch.nn.functional as F
from torch import nn

from ... import native
from ..util import build_MLP_layers, require_gpu, use_native
from .base import NCF
from .basic_ncf import _ScoringMixin


class RowsOf:
    """``table[index]`` left unevaluated: a (B, F) candidate batch that is a selection of rows of a resident feature
    table.  When the table is the very tensor passed as ``rated_items`` the model takes the candidates' embeddings from the
    catalogue embeddings it has already computed (``rated_emb[index]``: a 1 MB gather) instead of gathering B × F
    features and running the F -> IE Linear again (34 MB + 1.1 GFLOP per 4096-pair batch at config 3)."""

    def __init__(self, table: torch.Tensor, index: torch.Tensor):
        self.table, self.index = table, index

    @property
    def is_cuda(self):
        return self.table.is_cuda and self.index.is_cuda

    @property
    def device(self):
        return self.table.device

    @property
    def shape(self):
        return (self.index.shape[0], self.table.shape[1])

    def float(self):
        return self if self.table.dtype == torch.float32 else RowsOf(self.table.float(), self.index)

    def to(self, device):
        return self if self.table.device == torch.device(device) and self.index.device == torch.device(device) else RowsOf(self.table.to(device), self.index.to(device))

    def materialise(self) -> torch.Tensor:
        return self.table.index_select(0, self.index)


class SparseRatings:
    """CSR form of the (B, I) ``user_matrix``: row b owns entries [rowptr[b], rowptr[b+1]) with ``col`` = position in
    the rated-item list and ``val`` = the non-zero normalised rating.  Providers can emit this directly instead of
    the dense matrix (which is 2·B·I floats of mostly zeros).

    ``pair_row`` (optional, (B,) int64): the CSR then has one row per DISTINCT user of the batch and pair b uses row
    ``pair_row[b]`` — the dense matrix repeats a user's row for each of their pairs (dynamic_datasets.py:24-40); sharing
    it is what lets the LDS-tiled attention kernel stage a user's rated rows once for all of their pairs.

    ``max_row_len`` (optional, with ``pair_row``): an upper bound of the CSR's row lengths the HOST knows.  A training step then
    builds its per-pair CSR on the stream in buffers of B * max_row_len entries (native.pair_rows) instead of reading the entry
    count back; a row longer than the bound raises OverflowError at the epoch's flag check."""

    # below this average the per-pair kernel is used.  Measured at config-3 shapes (tools/ab_attn_grouped.py threshold),
    # grouped vs per-pair: 1 pair per set 335 vs 154 us, 2: 216 vs 153, 4: 128 vs 152, 8: 77 vs 151, 16+: 57 vs 147
    GROUPED_MIN_PAIRS_PER_ROW = 4

    def __init__(self, rowptr, col, val, num_items, pair_row=None, pairs_per_row_hint=None, max_row_len=None):
        self.rowptr, self.col, self.val, self.num_items = rowptr, col, val, int(num_items)
        self.pair_row = pair_row
        self.max_row_len = None if max_row_len is None else int(max_row_len)
        # average number of pairs per row IN USE, when the CSR holds more rows than the batch touches (a whole user
        # base kept on the GPU, pair_row = user position): the row count then says nothing about sharing
        self.pairs_per_row_hint = pairs_per_row_hint

    @property
    def pairs_per_row(self) -> float:
        if self.pairs_per_row_hint is not None:
            return float(self.pairs_per_row_hint)
        return self.num_pairs / max(1, int(self.rowptr.numel() - 1))

    @property
    def num_pairs(self) -> int:
        return int(self.pair_row.numel()) if self.pair_row is not None else int(self.rowptr.numel() - 1)

    def expanded(self) -> "SparseRatings":
        """Per-pair CSR (row b = pair b) of a shared-row instance; self if rows are not shared."""
        if self.pair_row is None:
            return self
        pr = self.pair_row.to(torch.int64)
        counts = (self.rowptr[1:] - self.rowptr[:-1])[pr]
        rowptr = torch.zeros(pr.numel() + 1, dtype=torch.int64, device=self.rowptr.device)
        rowptr[1:] = torch.cumsum(counts, 0)
        # entry k of pair b is entry rowptr_shared[pair_row[b]] + k of the shared arrays
        owner = torch.repeat_interleave(torch.arange(pr.numel(), device=pr.device), counts)
        src = self.rowptr[:-1][pr][owner] + (torch.arange(owner.numel(), device=pr.device) - rowptr[:-1][owner])
        ex = SparseRatings(rowptr, self.col[src].contiguous(), self.val[src].contiguous(), self.num_items)
        ex.shared_entry = src   # entry of the shared arrays each expanded entry came from
        return ex

    @staticmethod
    def from_dense(user_matrix: torch.Tensor, share_identical_rows: bool = True) -> "SparseRatings":
        """CSR of a dense (B, I) user matrix.  The reference's datasets repeat a user's row for each of their samples
        (dynamic_datasets.py:24-40) and its web backend passes ONE row repeated for every candidate
        (webapp/backend.py:78-121): with ``share_identical_rows`` rows that are exactly equal share one CSR row
        (``pair_row`` maps pairs to rows), which is what lets the LDS-tiled attention kernel stage a rated set once
        for all of its pairs.  Equal rows are found by a random projection (float64) and then VERIFIED element by
        element; a batch of mostly distinct rows skips the verification and keeps one row per pair.  (This function
        reads sizes back to the host in any case.)"""
        B = user_matrix.shape[0]
        if share_identical_rows and B > 1 and user_matrix.shape[1] > 0:
            gen = torch.Generator(device=user_matrix.device).manual_seed(0x5EED)
            proj = torch.rand(user_matrix.shape[1], dtype=torch.float64, device=user_matrix.device, generator=gen) + 0.5
            key = user_matrix.double() @ proj
            uniq, inv = torch.unique(key, return_inverse=True)
            R = int(uniq.numel())
            if R * SparseRatings.GROUPED_MIN_PAIRS_PER_ROW <= B:
                rep = torch.full((R,), B, dtype=torch.int64, device=user_matrix.device)
                rep.scatter_reduce_(0, inv, torch.arange(B, device=user_matrix.device), reduce="amin")   # first pair of each row
                if bool((user_matrix == user_matrix[rep][inv]).all()):
                    shared = SparseRatings.from_dense(user_matrix[rep], share_identical_rows=False)
                    shared.pair_row = inv.contiguous()
                    return shared
        mask = user_matrix != 0  # attention_ncf.py:158 — an entry that is exactly 0 counts as unrated
        rowptr = torch.zeros(user_matrix.shape[0] + 1, dtype=torch.int64, device=user_matrix.device)
        rowptr[1:] = torch.cumsum(mask.sum(dim=1), 0)
        nz = mask.nonzero()  # row-major: sorted by row, then by column
        return SparseRatings(rowptr, nz[:, 1].to(torch.int32).contiguous(), user_matrix[mask].float().contiguous(),
                             user_matrix.shape[1])

    @staticmethod
    def from_dense_on_stream(user_matrix: torch.Tensor, share_identical_rows: bool = True) -> "SparseRatings":
        """``from_dense`` without a single host read (libncf_hip.so: ncf_dense_csr_rows + a cumulative sum + ncf_dense_csr_fill, all
        on the current stream): rows that are exactly equal share one CSR row — found by a row hash, VERIFIED element by element on
        the device.  The CSR keeps B rows (a row that shares another's is empty) and ``col`` / ``val`` are sized for the worst case
        B * I, of which rowptr[B] entries are valid: sizes the host never learns.  What the host cannot know either is how much
        sharing there is; the reference's callers repeat rows (datasets/dynamic_datasets.py:24-40, webapp/backend.py:78-121), so the
        result carries ``pairs_per_row_hint`` = the grouped kernels' threshold: they are correct for any amount of sharing."""
        rowptr, col, val, pair_row = native.dense_to_csr(user_matrix.contiguous(), share_identical_rows)
        if not share_identical_rows:             # one CSR row per pair (the per-pair kernel's input): no indirection
            return SparseRatings(rowptr, col, val, user_matrix.shape[1])
        r = SparseRatings(rowptr, col, val, user_matrix.shape[1], pair_row=pair_row,
                          pairs_per_row_hint=SparseRatings.GROUPED_MIN_PAIRS_PER_ROW)
        r.nnz_hint = max(1, user_matrix.shape[1] // 4) * user_matrix.shape[0]     # for launch geometry only (slices per rated set)
        return r

    def to_dense(self, values: torch.Tensor) -> torch.Tensor:
        if self.pair_row is not None:
            ex = self.expanded()   # `values` may be aligned with the shared entries (e.g. self.val) or the expanded ones
            return ex.to_dense(values[ex.shared_entry] if values.numel() == self.col.numel() else values)
        B = self.rowptr.numel() - 1
        rows = torch.repeat_interleave(torch.arange(B, device=values.device), self.rowptr[1:] - self.rowptr[:-1])
        out = torch.zeros((B, self.num_items), dtype=values.dtype, device=values.device)
        out[rows, self.col.long()] = values
        return out


class AttentionNCF(_ScoringMixin, NCF):
    compatible_datasets = ("DynamicPointwiseDataset", "DynamicRankingDataset")
    # a dense (B, I) user_matrix is converted to shared-row CSR on the stream (no host read; the grouped kernels are used whatever the
    # sharing turns out to be).  False: round 2's conversion — two host reads, exact choice between the grouped and the per-pair kernel.
    dense_user_matrix_on_stream = True
    # True: a training step with message_dropout > 0 runs on the HIP attention kernels (ncf_attn_forward_train / _backward_train: the
    # entry mask is regenerated from a counter hash, not drawn from torch's Philox stream, so a seeded run draws other masks of the
    # same law).  False: that step takes the torch ops of _forward_train, as before.  A class attribute, not a kwarg: checkpoints
    # (get_model_parameters) stay the reference's.
    message_dropout_on_device = False

    def __init__(self, item_dim, item_emb=128, user_emb=128, att_dense=None, mlp_dense_layers=None,
                 use_cos_sim_instead=False, dropout_rate=0.2, message_dropout=None):
        super().__init__()
        if mlp_dense_layers is None:
            mlp_dense_layers = [256, 128]
        self.kwargs = {'item_dim': item_dim, 'item_emb': item_emb, 'user_emb': user_emb, 'att_dense': att_dense,
                       'mlp_dense_layers': mlp_dense_layers, 'dropout_rate': dropout_rate,
                       'use_cos_sim_instead': use_cos_sim_instead, 'message_dropout': message_dropout}
        self.use_cos_sim_instead = use_cos_sim_instead
        self.message_dropout = message_dropout
        self.ItemEmbeddings = nn.Sequential(nn.Linear(item_dim, item_emb))
        self.UserEmbeddings = nn.Sequential(nn.Linear(item_dim, user_emb))
        if not use_cos_sim_instead:
            if att_dense is not None:
                self.att_dense = att_dense
                self.AttentionNet = nn.Sequential(nn.Linear(2 * item_emb, att_dense), nn.ReLU(), nn.Dropout(dropout_rate),
                                                  nn.Linear(att_dense, 1))
            else:
                self.att_dense = 0
                self.AttentionNet = nn.Sequential(nn.Linear(2 * item_emb, 1))
        self.MLP = build_MLP_layers(item_emb + user_emb, mlp_dense_layers, dropout_rate=dropout_rate)

    def get_model_parameters(self) -> dict:
        return self.kwargs

    def important_hypeparams(self) -> str:
        return '_cosine' if self.use_cos_sim_instead else f'_attNet{self.att_dense}'

    # ------------------------------------------------------------------------------------------ HIP scoring
    def _att_split(self, cache=None):
        """Contiguous halves of AttentionNet.0 split at the cat(candidate, rated) boundary (:176).  With a hidden attention
        layer (att_dense) both halves and the bias carry the factor 2^-64 and AttentionNet's output weight 2^64
        (native.ATT_MLP_SCALED: w1 relu(pc + pr) is unchanged bit for bit — powers of two scale exactly — and in scaled
        units relu is the [0, 1] clamp of the kernel's packed add)."""
        cache = self._refresh() if cache is None else cache
        if "att_split" not in cache:
            l0 = self.AttentionNet[0]
            IE = self.ItemEmbeddings[0].out_features
            w = l0.weight.detach()
            f = 2.0 ** -native.ATT_SCALE_LOG2 if self.att_dense else 1.0
            cache["att_split"] = ((w[:, :IE] * f).contiguous(), (w[:, IE:] * f).contiguous(), (l0.bias.detach() * f).contiguous())
        return cache["att_split"]

    def _tail_mlp(self, cache):
        """(W1, b1, W2, b2, w3, b3) for ncf_attn_tail when the MLP has its shape (two hidden layers [256, 128] over item_emb = user_emb
        in {64, 128}: the class default and the shipped checkpoints), else None.  Cached per weight version (b3 is read once)."""
        if "tail_mlp" not in cache:
            from ..util import mlp_linears
            lins = mlp_linears(self.MLP)
            IE, UE = self.ItemEmbeddings[0].out_features, self.UserEmbeddings[0].out_features
            ok = (len(lins) == 3 and lins[2].out_features == 1 and not self.fold_first_layer
                  and native.attn_tail_supported(IE, UE, lins[0].out_features, lins[1].out_features))
            cache["tail_mlp"] = None
            if ok:
                # the two hidden layers' weights packed once per weight version in MFMA operand order (coalesced weight loads in the kernel)
                cache["tail_mlp"] = (native.PackedTailWeight(lins[0].weight.detach().contiguous()), lins[0].bias.detach().contiguous(),
                                     native.PackedTailWeight(lins[1].weight.detach().contiguous()), lins[1].bias.detach().contiguous(),
                                     lins[2].weight.detach().reshape(-1).contiguous(), float(lins[2].bias.detach().item()))
        return cache["tail_mlp"]

    def precompute_catalog(self, rated_items: torch.Tensor, cache=None):
        """Everything that depends only on the rated-item list: its embeddings, the rated half of the attention
        projection and the UserEmbeddings projection of the raw features.  Cached for the last list seen (serving
        scores one user against the whole catalogue, reference webapp/backend.py:78-121)."""
        cache = self._refresh() if cache is None else cache
        key = (rated_items.data_ptr(), tuple(rated_items.shape), rated_items._version)
        hit = cache.get("catalog")
        if hit is not None and hit[0] == key:
            return hit[1]
        x = rated_items.float().contiguous()
        li, lu = self.ItemEmbeddings[0], self.UserEmbeddings[0]
        rated_emb = native.linear(x, li.weight.detach(), li.bias.detach())
        if self.use_cos_sim_instead:
            pr = native.l2_normalize_rows(rated_emb)
        else:
            _, wr, _ = self._att_split(cache)
            pr = native.linear(rated_emb, wr, None)
        proj = native.linear(x, lu.weight.detach(), None)  # P = rated_items @ Wu^T ; bias added once per user row
        val = (rated_emb, pr, proj)
        cache["catalog"] = (key, val, rated_items)
        return val

    def forward(self, candidate_items, rated_items, user_matrix, return_attention_weights=False, pair_split=None):
        """``pair_split`` (``forward_pairs``): the batch is the positives' pairs followed by the negatives', split at that row."""
        if not use_native(self):
            if isinstance(candidate_items, RowsOf):
                candidate_items = candidate_items.materialise()
            return self._forward_train(candidate_items, rated_items, user_matrix, return_attention_weights, pair_split)
        require_gpu(candidate_items, rated_items)
        cache = self._refresh()  # ONE parameter fingerprint per forward (it walks the module tree: ~12 us of host time)
        li, lu = self.ItemEmbeddings[0], self.UserEmbeddings[0]
        rated_emb, pr, proj = self.precompute_catalog(rated_items, cache)
        pc_kept = None
        att_dense = 0 if self.use_cos_sim_instead else int(self.att_dense or 0)
        A_att = li.out_features if self.use_cos_sim_instead else (att_dense or 1)
        mode_att = native.ATT_COS if self.use_cos_sim_instead else (native.ATT_MLP_SCALED if att_dense else native.ATT_LINEAR)
        can_group = native.attn_grouped_supported(mode_att, A_att, lu.out_features)
        if isinstance(user_matrix, SparseRatings):
            ratings = user_matrix
        elif (user_matrix.is_cuda and user_matrix.dtype == torch.float32 and not return_attention_weights
              and 0 < user_matrix.numel() <= native.DENSE_CSR_MAX_ENTRIES and self.dense_user_matrix_on_stream):
            # the reference's call shape, no host round trip; rows are shared only where a grouped kernel can use the sharing
            ratings = SparseRatings.from_dense_on_stream(user_matrix, share_identical_rows=can_group)
        else:
            ratings = SparseRatings.from_dense(user_matrix)
        shared = ratings.pair_row is not None
        grouped = shared and can_group and ratings.pairs_per_row >= SparseRatings.GROUPED_MIN_PAIRS_PER_ROW
        grouping = None
        pc = None
        # never inside a HIP-graph capture: a hit would leave the candidate projections out of the captured graph
        keep = not isinstance(candidate_items, RowsOf) and not torch.cuda.is_current_stream_capturing()
        if isinstance(candidate_items, RowsOf):
            if candidate_items.table is rated_items:
                cand_emb = rated_emb.index_select(0, candidate_items.index)   # same Linear, already applied to every row
            else:
                cand_emb = native.linear(candidate_items.materialise().float().contiguous(), li.weight.detach(), li.bias.detach())
        else:
            # The candidate projections depend only on the candidate tensor and the weights: a serving loop scores every user
            # against the SAME catalogue tensor (webapp/backend.py:78-121), so the last one seen is kept (like the rated-item
            # catalogue above).  The key holds address, shape and version; the tensor itself is kept alive with the entry, so
            # the address cannot be recycled under it, and an in-place edit bumps the version.
            ckey = (candidate_items.data_ptr(), tuple(candidate_items.shape), candidate_items.dtype, candidate_items._version)
            kept = cache.get("candidates") if keep else None
            if kept is not None and kept[0] == ckey:
                cand_emb, pc_kept = kept[1], kept[2]
            elif att_dense and native.attn_candidates_supported(li.in_features, li.out_features, att_dense):
                # ONE launch: ItemEmbeddings on the candidates, their half of AttentionNet.0, and (in a spare workgroup) the
                # batch's pairs listed by rated set for the grouped attention kernel
                wc, _, b0 = self._att_split(cache)
                B = candidate_items.shape[0]
                R = ratings.rowptr.numel() - 1
                fuse_grouping = grouped and not return_attention_weights and B <= 32768 and R <= 32768
                ppw = native.default_pairs_per_wg(B)
                if "cand_packed" not in cache:       # ItemEmbeddings' weight in MFMA operand order: once per weight version
                    cache["cand_packed"] = native.PackedCandidateWeight(li.weight.detach())
                cand_emb, pc, grouping = native.attn_candidates(
                    candidate_items.float().contiguous(), cache["cand_packed"], li.bias.detach(), wc, b0,
                    ratings.pair_row.to(torch.int64).contiguous() if fuse_grouping else None, R, ppw)
                if grouping is not None:
                    grouping = (grouping, ppw)
            else:
                cand_emb = native.linear(candidate_items.float().contiguous(), li.weight.detach(), li.bias.detach())
        if pc is not None:
            pass
        elif pc_kept is not None:
            pc = pc_kept
        elif self.use_cos_sim_instead:
            pc = native.l2_normalize_rows(cand_emb)
        else:
            wc, _, b0 = self._att_split(cache)
            pc = native.linear(cand_emb, wc, b0)
        if keep and pc_kept is None:
            cache["candidates"] = (ckey, cand_emb, pc, candidate_items)
        if self.use_cos_sim_instead:
            mode, w1, b1 = native.ATT_COS, None, 0.0
        else:
            if self.att_dense:
                l1 = self.AttentionNet[-1]
                if "att_out" not in cache:
                    cache["att_out"] = ((l1.weight.detach().reshape(-1) * 2.0 ** native.ATT_SCALE_LOG2).contiguous(),
                                        float(l1.bias.detach().item()))
                w1, b1 = cache["att_out"]
                mode = native.ATT_MLP_SCALED
            else:
                mode, w1, b1 = native.ATT_LINEAR, None, 0.0
        if grouped:
            # several pairs per rated set: stage each set once per workgroup in LDS (K3 grouped form)
            tail = None if return_attention_weights else self._tail_mlp(cache)
            res = native.attn_forward_grouped(mode, pc, pr, w1, b1, ratings.rowptr, ratings.col, ratings.val,
                                              ratings.pair_row, proj, out_bias=lu.bias.detach(),
                                              return_weights=return_attention_weights, grouping=grouping,
                                              nnz_hint=getattr(ratings, "nnz_hint", None), leave_partials=tail is not None)
            if tail is not None:
                # ONE launch: merge of the attention's partials (+ UserEmbeddings' bias), cat(candidate_emb, user_emb), MLP (:208-222)
                parts = isinstance(res, native.AttnPartials)
                return native.attn_tail(cand_emb, res, lu.bias.detach() if parts else None, *tail)
            if return_attention_weights:
                out = self._score(cand_emb, None, res[0], None, cache=cache)
                return out, ratings.expanded().to_dense(res[1])
            return self._score(cand_emb, None, res, None, cache=cache)
        if shared:
            ratings = ratings.expanded()
        user_emb, wts = native.attn_forward(mode, pc, pr, w1, b1, ratings.rowptr, ratings.col, ratings.val, proj,
                                            out_bias=lu.bias.detach())
        out = self._score(cand_emb, None, user_emb, None, cache=cache)  # cat(candidate_emb, user_emb): :219
        if return_attention_weights:
            return out, ratings.to_dense(wts)
        return out

    # ------------------------------------------------------------------------------------------ many users x one catalogue
    # largest logit table (4 * I_c * I_c bytes) the cross-product route builds: 1 GiB is a catalogue of about 16k items
    cross_table_max_bytes = 1 << 30
    # one block of catalogue_scores: the user_emb rows (4 * UE bytes per pair), the scores and the item position of each pair
    CATALOGUE_BLOCK_BYTES = 256 << 20

    def _att_out(self, cache):
        """(mode, w1, b1) of the attention kernels for this model, as ``forward`` passes them."""
        if self.use_cos_sim_instead:
            return native.ATT_COS, None, 0.0
        if not self.att_dense:
            return native.ATT_LINEAR, None, 0.0
        if "att_out" not in cache:
            l1 = self.AttentionNet[-1]
            cache["att_out"] = ((l1.weight.detach().reshape(-1) * 2.0 ** native.ATT_SCALE_LOG2).contiguous(), float(l1.bias.detach().item()))
        return (native.ATT_MLP_SCALED,) + cache["att_out"]

    def cross_route(self, n_items: int, table=None) -> bool:
        """Whether ``catalogue_scores`` over a catalogue of ``n_items`` takes the logit-table route.  ``table=None``: where the cross
        kernel has an instance for ``user_emb`` and the table fits ``cross_table_max_bytes``; ``True`` outside those limits raises
        ValueError; ``False`` is the pair route.  Host only."""
        if table is False:
            return False
        UE = self.UserEmbeddings[0].out_features
        nbytes = 4 * int(n_items) * int(n_items)
        fits, shape = nbytes <= self.cross_table_max_bytes, native.attn_cross_supported(UE)
        if table and not fits:
            raise ValueError(f"the logit table of {n_items} items takes {nbytes} bytes, above AttentionNCF.cross_table_max_bytes = "
                             f"{self.cross_table_max_bytes}")
        if table and not shape:
            raise ValueError(f"the cross-product attention kernel has no instance for user_emb = {UE} (a multiple of 32 in 32 .. 256)")
        return fits and shape

    def logit_table(self, item_features: torch.Tensor, cache=None):
        """ST (I_c, I_c): the attention logit of every (rated item, candidate) pair of the catalogue (native.attn_logits), kept per
        weight version for the last catalogue tensor seen beside ``precompute_catalog``'s entry (key: address, shape, version)."""
        cache = self._refresh() if cache is None else cache
        key = (item_features.data_ptr(), tuple(item_features.shape), item_features._version)
        hit = cache.get("cross_table")
        if hit is not None and hit[0] == key:
            return hit[1]
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the logit table is never built inside a stream capture: call catalogue_scores once before capturing")
        rated_emb, pr, _ = self.precompute_catalog(item_features, cache)
        if self.use_cos_sim_instead:
            pc = native.l2_normalize_rows(rated_emb)
        else:
            wc, _, b0 = self._att_split(cache)
            pc = native.linear(rated_emb, wc, b0)          # the candidates ARE the catalogue: same ItemEmbeddings rows
        mode, w1, b1 = self._att_out(cache)
        ST = native.attn_logits(mode, pc, pr, w1, b1)
        cache["cross_table"] = (key, ST, item_features)
        return ST

    def catalogue_score_blocks(self, item_features, ratings, user_rows, item_ids=None, table=None, block_bytes=None):
        """Yields ``(u0, u1, scores (u1 - u0, I))`` of ``catalogue_scores``, in blocks of users whose user_emb rows, scores and
        item positions stay under ``block_bytes``.  Nothing synchronises with the host."""
        if self.training:
            raise RuntimeError("catalogue_scores is computed in eval mode: call model.eval() first")
        if not isinstance(ratings, SparseRatings):
            raise TypeError("ratings must be a SparseRatings whose rows are users and whose columns are catalogue positions")
        if item_features.dim() != 2 or ratings.num_items != item_features.shape[0]:
            raise ValueError(f"ratings has {ratings.num_items} columns, the catalogue {tuple(item_features.shape)} rows")
        if user_rows.dtype != torch.int64 or user_rows.dim() != 1:
            raise ValueError("user_rows must be a 1-D int64 tensor of rows of ratings")
        if item_ids is not None and (item_ids.dtype != torch.int64 or item_ids.dim() != 1):
            raise ValueError("item_ids must be a 1-D int64 tensor of catalogue positions")
        Ic = item_features.shape[0]
        use_table = self.cross_route(Ic, table)
        require_gpu(item_features, ratings.rowptr, ratings.col, ratings.val, user_rows, item_ids)
        lu = self.UserEmbeddings[0]
        UE = lu.out_features
        I = Ic if item_ids is None else item_ids.numel()
        U = user_rows.numel()
        user_rows = user_rows.contiguous()
        block_bytes = self.CATALOGUE_BLOCK_BYTES if block_bytes is None else int(block_bytes)
        rows_per_block = max(1, block_bytes // max(1, I * (4 * UE + 4 + 8)))
        with torch.no_grad():
            cache = self._refresh()
            if use_table and table is None and torch.cuda.is_current_stream_capturing() and cache.get("cross_table") is None:
                use_table = False
            items = torch.arange(Ic, dtype=torch.int64, device=item_features.device) if item_ids is None else item_ids.contiguous()
            if use_table:
                ST = self.logit_table(item_features, cache)
                rated_emb, _, proj = self.precompute_catalog(item_features, cache)
                bias = lu.bias.detach()
        pos, pos_n = None, -1
        for u0 in range(0, U, rows_per_block):
            u1 = min(U, u0 + rows_per_block)
            nb = u1 - u0
            with torch.no_grad():
                if I == 0:
                    scores = torch.empty((nb, 0), dtype=torch.float32, device=item_features.device)
                elif use_table:
                    if pos_n != nb:
                        pos, pos_n = items.repeat(nb), nb
                    user_emb = native.attn_cross(ST, ratings.rowptr, ratings.col, ratings.val, user_rows[u0:u1], proj, out_bias=bias,
                                                 cand_ids=None if item_ids is None else items)
                    # the fused scorer with an index on table A: cat(candidate_emb, user_emb) -> MLP (:219-222)
                    scores = self._score(rated_emb, pos, user_emb, None, cache=cache).view(nb, I)
                else:
                    pairs = SparseRatings(ratings.rowptr, ratings.col, ratings.val, ratings.num_items,
                                          pair_row=user_rows[u0:u1].repeat_interleave(I), pairs_per_row_hint=I)
                    scores = self.forward(RowsOf(item_features, items.repeat(nb)), item_features, pairs).view(nb, I)
            yield u0, u1, scores                  # outside the with: a suspended generator must not hold the grad mode

    def catalogue_scores(self, item_features, ratings, user_rows, item_ids=None, table=None, block_bytes=None):
        """(U, I) fp32 scores of the users ``user_rows`` (rows of ``ratings``) against the catalogue ``item_features`` (I_c, F) — all
        of it, or the positions ``item_ids`` — where the catalogue is both the candidate list and the rated-item list: what the
        reference computes one user per request (webapp/backend.py:78-121).  Eval only.  ratings: a SparseRatings whose rows are
        users and whose columns are catalogue positions (``pair_row`` unused), e.g. a ``SparseDynamicProvider.device_state``.

        table=True: the cross-product route.  The attention logits depend on (candidate, rated item) only, so they are ONE (I_c, I_c)
        table per weight version and catalogue (``logit_table``; native.attn_logits) and a user's attention is a lookup plus a
        softmax-weighted sum on the matrix cores (native.attn_cross); the MLP tail is the fused scorer ``forward`` ends with.
        table=False: the same blocks as (user, item) pairs through ``forward`` (the grouped kernels).  table=None: the table where
        the cross kernel takes ``user_emb`` and 4 * I_c^2 <= ``cross_table_max_bytes``, else the pair route.  The two routes
        agree to fp32 summation order."""
        blocks = [s for _, _, s in self.catalogue_score_blocks(item_features, ratings, user_rows, item_ids, table, block_bytes)]
        if not blocks:
            I = item_features.shape[0] if item_ids is None else item_ids.numel()
            return torch.empty((0, I), dtype=torch.float32, device=item_features.device)
        return blocks[0] if len(blocks) == 1 else torch.cat(blocks)

    def explain(self, item_features, ratings, user_rows, items, thr, max_reasons):
        """The reasons behind recommendations, for many users at once: ``(positions (U, k, E) int32, weights (U, k, E) fp32, ratings
        (U, k, E) fp32, counts (U, k) int32)`` with E = ``max_reasons`` — per (user, slot) the rated items of user ``user_rows[u]``
        whose attention weight towards catalogue position ``items[u, s]`` exceeds ``thr[u]``, in descending weight, ``counts``
        uncapped, unused slots ``(-1, 0, 0)`` (native.attn_explain; the reference thresholds one user's dense weight rows on the host,
        webapp/backend.py:105-121).  Eval only.  ``ratings`` as in ``catalogue_scores``; ``items`` (U, k) int64 catalogue positions
        with -1 for an empty slot; ``thr`` (U,) fp32.  Reads ``logit_table(item_features)`` only — any ``user_emb`` width — so the
        table must fit ``cross_table_max_bytes``.  Nothing synchronises with the host."""
        if self.training:
            raise RuntimeError("explanations are computed in eval mode: call model.eval() first")
        if not isinstance(ratings, SparseRatings):
            raise TypeError("ratings must be a SparseRatings whose rows are users and whose columns are catalogue positions")
        if item_features.dim() != 2 or ratings.num_items != item_features.shape[0]:
            raise ValueError(f"ratings has {ratings.num_items} columns, the catalogue {tuple(item_features.shape)} rows")
        if user_rows.dtype != torch.int64 or user_rows.dim() != 1:
            raise ValueError("user_rows must be a 1-D int64 tensor of rows of ratings")
        U = user_rows.numel()
        if items.dtype != torch.int64 or items.dim() != 2 or items.shape[0] != U:
            raise ValueError(f"items must be a ({U}, k) int64 tensor of catalogue positions (-1: an empty slot)")
        if thr.dtype != torch.float32 or thr.dim() != 1 or thr.numel() != U:
            raise ValueError(f"thr must be a ({U},) fp32 tensor: one threshold per listed user")
        if not 1 <= int(max_reasons) <= native.ATTN_EXPLAIN_MAX_REASONS:
            raise ValueError(f"max_reasons = {max_reasons} is outside 1 .. {native.ATTN_EXPLAIN_MAX_REASONS}")
        Ic = item_features.shape[0]
        nbytes = 4 * Ic * Ic
        if nbytes > self.cross_table_max_bytes:
            raise ValueError(f"the logit table of {Ic} items takes {nbytes} bytes, above AttentionNCF.cross_table_max_bytes = "
                             f"{self.cross_table_max_bytes}")
        require_gpu(item_features, ratings.rowptr, ratings.col, ratings.val, user_rows, items, thr)
        with torch.no_grad():
            ST = self.logit_table(item_features)       # raises inside a stream capture when no table has been built
            return native.attn_explain(ST, ratings.rowptr, ratings.col, ratings.val, user_rows.contiguous(), items.contiguous(),
                                       thr.contiguous(), int(max_reasons))

    def attention_stats(self, item_features, ratings, user_rows, cands, out=None):
        """The item-item attention statistics of a sample file: ``(sum (I_c, I_c) float64, count (I_c, I_c) int64)`` where, for every
        sample (user ``user_rows[s]``, candidate ``cands[s]``) and every rated item j of that user, ``sum[cand, j]`` collects the
        attention weight of j towards the candidate and ``count[cand, j]`` the number of such samples — the tables the reference's
        evaluation keeps for its attention heat-map (eval.py:101-108, 137-143), without a dense (samples, I_c) weight matrix
        (native.attn_stats).  Eval only.  ``ratings`` as in ``catalogue_scores`` (a row lists a catalogue position once);
        ``user_rows`` and ``cands`` (S,) int64.  ``out``: ``(sum, count)`` of an earlier call to continue — the additions into a cell
        happen in sample order from the value already there, so a file fed in consecutive pieces gives the bits of one call; zeroed
        tables are allocated without it.  Reads ``logit_table(item_features)`` only, so the table must fit ``cross_table_max_bytes``.
        Nothing synchronises with the host."""
        if self.training:
            raise RuntimeError("attention statistics are computed in eval mode: call model.eval() first")
        if not isinstance(ratings, SparseRatings):
            raise TypeError("ratings must be a SparseRatings whose rows are users and whose columns are catalogue positions")
        if item_features.dim() != 2 or ratings.num_items != item_features.shape[0]:
            raise ValueError(f"ratings has {ratings.num_items} columns, the catalogue {tuple(item_features.shape)} rows")
        if user_rows.dtype != torch.int64 or user_rows.dim() != 1:
            raise ValueError("user_rows must be a 1-D int64 tensor of rows of ratings")
        S = user_rows.numel()
        if not torch.is_tensor(cands) or cands.dtype != torch.int64 or cands.dim() != 1 or cands.numel() != S:
            raise ValueError(f"cands must be a ({S},) int64 tensor of catalogue positions: one candidate per sample")
        Ic = item_features.shape[0]
        if out is not None:
            if not (isinstance(out, (tuple, list)) and len(out) == 2 and all(torch.is_tensor(o) and tuple(o.shape) == (Ic, Ic) for o in out)
                    and out[0].dtype == torch.float64 and out[1].dtype == torch.int64):
                raise ValueError(f"out must be (sum ({Ic}, {Ic}) float64, count ({Ic}, {Ic}) int64)")
        nbytes = 4 * Ic * Ic
        if nbytes > self.cross_table_max_bytes:
            raise ValueError(f"the logit table of {Ic} items takes {nbytes} bytes, above AttentionNCF.cross_table_max_bytes = "
                             f"{self.cross_table_max_bytes}")
        require_gpu(item_features, ratings.rowptr, ratings.col, user_rows, cands, *(out or ()))
        with torch.no_grad():
            ST = self.logit_table(item_features)       # raises inside a stream capture when no table has been built
            if out is None:
                out = (torch.zeros((Ic, Ic), dtype=torch.float64, device=ST.device), torch.zeros((Ic, Ic), dtype=torch.int64, device=ST.device))
            return native.attn_stats(ST, ratings.rowptr.contiguous(), ratings.col.contiguous(), user_rows.contiguous(), cands.contiguous(),
                                     out[0], out[1])

    # ------------------------------------------------------------------------------------------ torch training path
    def _forward_train_hip(self, candidate_items, rated_items, user_matrix, return_attention_weights, pair_split=None):
        """attention_ncf.py:136-224 with autograd recording, on the HIP blocks: the Linear layers (LinearFn), the attention with its
        softmax and weighted sum (AttnFn: forward and backward kernels; AttentionNet's hidden dropout regenerated from a hash in
        both; with message_dropout_on_device the message dropout over the logits too), the MLP (mlp_train).  The train-only target masking (:195-205, a candidate must not attend to itself) is decided
        per rated ENTRY with the reference's own test (isclose of the two embedding rows) and applied by dropping the entry."""
        from ...autograd import AttnFn, LinearFn, mlp_train
        li, lu = self.ItemEmbeddings[0], self.UserEmbeddings[0]
        cand = candidate_items.float().contiguous()
        rated = rated_items.float().contiguous()
        cand_emb = LinearFn.apply(cand, li.weight, li.bias, False)
        rated_emb = LinearFn.apply(rated, li.weight, li.bias, False)
        ratings = user_matrix if isinstance(user_matrix, SparseRatings) else SparseRatings.from_dense(user_matrix, share_identical_rows=False)
        on_stream = (ratings.pair_row is not None and ratings.max_row_len is not None and not return_attention_weights
                     and ratings.rowptr.is_cuda)
        if on_stream:
            # per-pair CSR and target mask in one pass on the stream (ncf_pair_rows_*): no size reaches the host, the buffers are
            # sized by the host's bound and the kernels downstream are bounded by rowptr
            mask = (cand_emb.detach(), rated_emb.detach()) if self.training else None
            rowptr, col, val, _ = native.pair_rows(ratings.rowptr, ratings.col, ratings.val, ratings.pair_row.to(torch.int64).contiguous(),
                                                   ratings.pair_row.numel() * ratings.max_row_len, mask,
                                                   flag=native._pair_rows_flag(ratings.rowptr.device))
        elif ratings.pair_row is not None:
            ratings = ratings.expanded()
        if not on_stream:
            rowptr, col, val = ratings.rowptr, ratings.col, ratings.val
        if not on_stream and self.training and col.numel():
            b_of = torch.repeat_interleave(torch.arange(rowptr.numel() - 1, device=col.device), rowptr[1:] - rowptr[:-1])
            same = torch.isclose(cand_emb.detach()[b_of], rated_emb.detach()[col.long()], atol=1e-5).all(dim=1)
            col = torch.where(same, torch.full_like(col, -1), col)        # a dropped entry: score -inf, weight 0 (:192-205)
        dropout = None
        hidden_seed, msg_seed = self._draw_attention_seeds()
        if self.use_cos_sim_instead:
            mode, w1, b1 = native.ATT_COS, None, None
            pc, pr = F.normalize(cand_emb, p=2, dim=1), F.normalize(rated_emb, p=2, dim=1)
        else:
            l0, l1 = self.AttentionNet[0], self.AttentionNet[-1]
            IE = li.out_features
            pc = LinearFn.apply(cand_emb, l0.weight[:, :IE], l0.bias, False)      # AttentionNet.0 split at the cat boundary (:176)
            pr = LinearFn.apply(rated_emb, l0.weight[:, IE:], None, False)
            mode, w1, b1 = native.ATT_MLP, l1.weight.view(-1), l1.bias
            if hidden_seed is not None:
                dropout = (float(self.AttentionNet[2].p), hidden_seed)
        proj = LinearFn.apply(rated, lu.weight, None, False)        # UserEmbeddings is linear over the weighted sum (:212-216)
        msg_dropout = None if msg_seed is None else (float(self.message_dropout), msg_seed)
        user_emb, wts = AttnFn.apply(pc, pr, w1, b1, proj, lu.bias, rowptr, col, val, mode, dropout, msg_dropout)
        out = self._train_mlp(torch.cat((cand_emb, user_emb), dim=1), True, pair_split)
        if return_attention_weights:
            dense = SparseRatings(rowptr, ratings.col, val, ratings.num_items).to_dense(wts.detach())
            return out, dense
        return out

    def _message_dropout_active(self):
        return bool(self.training and self.message_dropout)

    def _draw_attention_seeds(self):
        """(hidden seed or None, message seed or None) of one step on the HIP blocks, from the host generator (no device sync).  The
        hidden seed is drawn first and only when AttentionNet's hidden dropout is active; the message seed after it and only when
        the message dropout runs on the device — so a run without message_dropout_on_device consumes the generator as before."""
        hidden = msg = None
        if not self.use_cos_sim_instead and self.att_dense:
            drop = self.AttentionNet[2]
            if self.training and isinstance(drop, nn.Dropout) and drop.p > 0:
                hidden = native.host_seed()
        if self._message_dropout_active() and self.message_dropout_on_device:
            msg = native.host_seed()
        return hidden, msg

    def _forward_train(self, candidate_items, rated_items, user_matrix, return_attention_weights, pair_split=None):
        hip = (candidate_items.is_cuda and not getattr(self, "train_with_torch_ops", False)
               and (self.message_dropout_on_device or not self._message_dropout_active())
               and (self.use_cos_sim_instead or self.att_dense) and native.attn_backward_supported(
                   native.ATT_COS if self.use_cos_sim_instead else native.ATT_MLP,
                   self.ItemEmbeddings[0].out_features if self.use_cos_sim_instead else int(self.att_dense), self.UserEmbeddings[0].out_features))
        if hip:
            return self._forward_train_hip(candidate_items, rated_items, user_matrix, return_attention_weights, pair_split)
        if isinstance(user_matrix, SparseRatings):
            user_matrix = user_matrix.expanded()
            user_matrix = user_matrix.to_dense(user_matrix.val)
        B, I = candidate_items.shape[0], rated_items.shape[0]
        cand_emb = self.ItemEmbeddings(candidate_items)
        rated_emb = self.ItemEmbeddings(rated_items)
        valid = user_matrix != 0
        pairs = valid.nonzero()
        c, r = cand_emb[pairs[:, 0]], rated_emb[pairs[:, 1]]
        if self.use_cos_sim_instead:
            att = (F.normalize(c, p=2, dim=1) * F.normalize(r, p=2, dim=1)).sum(dim=1)
        else:
            att = self.AttentionNet(torch.cat((c, r), dim=1)).view(-1)
        if self.training and self.message_dropout is not None:
            att = F.dropout(att, p=self.message_dropout, training=True)
            att = torch.where(att == 0, torch.full_like(att, -float('inf')), att)
        scores = torch.full((B, I), -float('inf'), dtype=att.dtype, device=att.device)     # fp32, or fp64 for a .double() module
        scores[valid] = att
        if self.training:
            # the candidate itself must not attend to itself while fitting its rating (:195-205)
            try:
                same = torch.isclose(cand_emb.unsqueeze(1), rated_emb.unsqueeze(0), atol=1e-5).all(dim=2)
                scores = scores.masked_fill(same, -float('inf'))
            except Exception:  # the reference only warns here
                print("Warning: Could not calculate training mask. Ignoring masking this time.", file=sys.stderr)
        scores = F.softmax(scores, dim=1).nan_to_num(nan=0.0, posinf=0.0, neginf=0.0)
        user_feat = torch.matmul(scores * user_matrix, rated_items)
        user_emb = self.UserEmbeddings(user_feat)
        out = self._train_mlp(torch.cat((cand_emb, user_emb), dim=1), False, pair_split)
        return (out, scores.detach()) if return_attention_weights else out

    # ------------------------------------------------------------------------------------------ pair-wise step in one forward
    def _train_mlp(self, x, hip, pair_split=None):
        """The MLP of a training step.  With ``pair_split`` it is applied to the two halves of the batch separately (everything
        before it — the catalogue-side Linears above all — runs once over all 2B rows)."""
        from ...autograd import mlp_train
        run = (lambda t: mlp_train(self.MLP, t)) if hip else self.MLP
        return run(x) if pair_split is None else torch.cat((run(x[:pair_split]), run(x[pair_split:])), dim=0)

    def forward_pairs(self, candidate_items, rated_items, user_matrix, split):
        """(out[:split], out[split:]) of ONE forward over the positives' pairs followed by the negatives' (a pair-wise step: the
        rated items' embeddings and projections are computed once instead of once per call).  In a training step the MLP is applied
        to the two halves separately, as two forwards would.  Under the BPR loss the gradient of out_neg is exactly minus that of
        out_pos, so the output bias — and the bias of every hidden unit that is active for all pairs — has a gradient that is
        exactly zero: two column sums over g and -g add up to that zero, where one column sum over [g; -g] leaves rounding noise,
        which Adam turns into steps of lr (measured: MLP.0.bias 4e-2 of its largest element off after 16 steps)."""
        out = self(candidate_items, rated_items, user_matrix, pair_split=int(split))
        return out[:split], out[split:]
