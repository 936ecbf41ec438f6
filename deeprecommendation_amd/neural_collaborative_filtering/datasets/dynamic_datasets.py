"""DynamicPointwiseDataset / DynamicRankingDataset (reference datasets/dynamic_datasets.py): the user profile is built per
batch from the user's rated items by the provider's ``collate_interacted_items``."""
import numpy as np
import torch

from .base import NegativeSampler, PointwiseDataset, RankingDataset, ResidentInputs, ResidentPairs
from ..models.attention_ncf import RowsOf, SparseRatings


def _dev(x, device):
    if isinstance(x, SparseRatings):
        return SparseRatings(x.rowptr.to(device), x.col.to(device), x.val.to(device), x.num_items,
                             None if x.pair_row is None else x.pair_row.to(device), x.pairs_per_row_hint, x.max_row_len)
    return x.float().to(device)


def _pairs_per_user(users, batch_size):
    """Pairs per distinct user in a batch, estimated on a few batches of the file (decides grouped vs per-pair kernel)."""
    bs = int(batch_size or 512)
    starts = np.unique(np.linspace(0, max(0, len(users) - bs), num=8).astype(np.int64))
    return float(np.mean([len(users[s:s + bs]) / max(1, len(np.unique(users[s:s + bs]))) for s in starts])) if len(users) else 1.0


class DynamicPointwiseDataset(PointwiseDataset):
    resident_opt_in = True      # train_model builds batches on the device only with resident=True (None keeps the DataLoader loop)

    def __init__(self, file_or_frame, dynamic_provider):
        super().__init__(file_or_frame)
        self.dynamic_provider = dynamic_provider

    def use_collate(self):
        return lambda batch: self.dynamic_provider.collate_interacted_items(batch, for_ranking=False)

    def resident_inputs(self, device=None, batch_size=None):
        """Raw (user id, candidate id) columns; each batch becomes the collate's 6-tuple ON THE GPU from the provider's
        device-resident state (feature table, every user's rated set as one CSR): see SparseDynamicProvider.device_state."""
        dp = self.dynamic_provider
        if device is None or not hasattr(dp, "device_state") or not getattr(dp, "sparse", False):
            return None
        state = dp.device_state(device)
        if state is None or not (np.issubdtype(self._u.dtype, np.integer) and np.issubdtype(self._i.dtype, np.integer)):
            return None
        hint = _pairs_per_user(self._u, batch_size)

        def on_batch(upos, cpos, y):
            return state.batch_at(upos, cpos, y, hint)

        def train_on_batch(upos, cpos, y):
            return state.train_batch_at(upos, cpos, y, hint)

        # id -> position once per uploaded chunk (a dozen small torch kernels), the batch tuple per batch
        return ResidentInputs((torch.as_tensor(self._u, dtype=torch.int64), torch.as_tensor(self._i, dtype=torch.int64)),
                              self._targets(), on_chunk=state.positions, on_batch=on_batch,
                              train_on_chunk=state.train_positions, train_on_batch=train_on_batch)

    @staticmethod
    def do_forward(model, batch, device, return_attention_weights=False):
        cand_ids, rated_ids, candidate_items, rated_items, user_matrix, y_batch = batch
        res = model(candidate_items.float().to(device), rated_items.float().to(device), _dev(user_matrix, device),
                    return_attention_weights=return_attention_weights)
        if return_attention_weights:
            out, att = res
            return out, y_batch, cand_ids, rated_ids, att, user_matrix
        return res, y_batch


class DynamicResidentPairs(ResidentPairs):
    """ResidentPairs over a SparseDynamicProvider's device state: ``batch`` is the collate's ``for_ranking`` 6-tuple built on the
    device — (positive positions, None, RowsOf(features, positives), features, ratings, RowsOf(features, negatives)); ``users`` are
    rows of the state's CSR."""

    def __init__(self, dataset, state, users, positives, sampler, hint):
        super().__init__(dataset, users, positives, sampler)
        self.state, self.hint = state, hint

    def batch(self, pick, seed, slot0):
        pick = pick.contiguous()
        st = self.state
        pos = self.positives[pick]
        neg = self.sampler.draw(pick, self.dataset.w, seed, slot0).clamp_min(0)     # -1 (a bad pick) is flagged by the sampler
        return pos, None, RowsOf(st.features, pos), st.features, st.train_ratings(self.users[pick], self.hint), RowsOf(st.features, neg)

    def check(self):
        from ... import native
        native.check_pair_rows(self.users.device)
        super().check()


class DynamicRankingDataset(RankingDataset):
    """Reference dynamic_datasets.py:43-61: the provider's collate with ``for_ranking=True`` (the negative's profile in the last
    slot), two model calls per batch; the DataLoader loop (negatives drawn on the host) unless train_model is asked for
    ``resident=True`` (``resident_pairs``)."""
    resident_opt_in = True

    def __init__(self, file_or_frame, dynamic_provider):
        super().__init__(file_or_frame)
        self.dynamic_provider = dynamic_provider

    def use_collate(self):
        return lambda batch: self.dynamic_provider.collate_interacted_items(batch, for_ranking=True)

    def resident_pairs(self, device=None, batch_size=None):
        """Over a SparseDynamicProvider with a device state: the user / positive id columns and the negatives' ids go up once and
        become CSR rows / catalogue positions once, on the device (an unknown id raises the sticky out-of-range flag: IndexError at
        the epoch's check); a batch is three gathers plus one ``sample_negatives`` call."""
        dp = self.dynamic_provider
        if device is None or torch.device(device).type != "cuda" or not hasattr(dp, "device_state") or not getattr(dp, "sparse", False):
            return None
        key = str(device)
        if key in self._resident:
            return self._resident[key]
        if not all(np.issubdtype(a.dtype, np.integer) for a in (self._u, self._pos, self._neg_ids)):
            return None
        state = dp.device_state(device)
        if state is None:
            return None
        dev = torch.device(device)
        users, positives = state.train_positions(torch.from_numpy(self._u.astype(np.int64)).to(dev),
                                                 torch.from_numpy(self._pos.astype(np.int64)).to(dev))
        negs = state.item_positions(torch.from_numpy(self._neg_ids.astype(np.int64)).to(dev))
        sampler = NegativeSampler(torch.from_numpy(self._rowptr).to(dev), negs, torch.from_numpy(self._neg_r.astype(np.float32)).to(dev))
        self._resident[key] = DynamicResidentPairs(self, state, users.contiguous(), positives.contiguous(), sampler,
                                                   _pairs_per_user(self._u, batch_size))
        return self._resident[key]

    @staticmethod
    def do_forward(model, batch, device):
        cand_ids, rated_ids, candidate_items1, rated_items, user_matrix, candidate_items2 = batch
        if (isinstance(candidate_items1, RowsOf) and isinstance(candidate_items2, RowsOf) and candidate_items1.table is candidate_items2.table
                and isinstance(user_matrix, SparseRatings) and user_matrix.pair_row is not None):
            # device-built batch: positives and negatives in ONE forward of 2B pairs (the catalogue-side Linears — the rated items'
            # embeddings and their two projections — run once per step instead of twice); pair b and pair B + b share a rated set
            B = candidate_items1.index.numel()
            um = user_matrix
            hint = None if um.pairs_per_row_hint is None else 2 * um.pairs_per_row_hint
            both = SparseRatings(um.rowptr, um.col, um.val, um.num_items, torch.cat((um.pair_row, um.pair_row)), hint, um.max_row_len)
            cand = RowsOf(candidate_items1.table, torch.cat((candidate_items1.index, candidate_items2.index)))
            return model.forward_pairs(cand.float().to(device), rated_items.float().to(device), _dev(both, device), B)
        rated, um = rated_items.float().to(device), _dev(user_matrix, device)
        out1 = model(candidate_items1.float().to(device), rated, um)
        out2 = model(candidate_items2.float().to(device), rated, um)
        return out1, out2
