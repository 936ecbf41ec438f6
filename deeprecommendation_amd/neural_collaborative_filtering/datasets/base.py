"""Dataset contracts of the reference (datasets/base.py): point-wise (userId, movieId, rating) triplets (:8-42) and pair-wise
(user, positive, sampled negative) triplets with the BPR loss (:45-99), each with a ``use_collate()`` hook, a static
``do_forward(model, batch, device, ...)`` and ``calculate_loss``."""
import numpy as np
import pandas as pd
import torch
from torch import nn, softmax
from torch.utils.data import Dataset


class ResidentInputs:
    """Whole-file model inputs for eval_model's device-resident loop: host ``tensors`` (sample order) + ``targets``;
    ``on_chunk(*device_tensors) -> inputs`` runs once per uploaded chunk (raw ids -> table positions), ``on_batch(*inputs,
    y) -> batch`` builds the tuple ``do_forward`` receives (default: ``(*inputs, y)``).  ``train_on_chunk`` / ``train_on_batch``:
    what train_model's resident loop uses in their place when given — it uploads the file once and keeps the chunk's inputs for
    every epoch, so they must not depend on state an evaluation pass between two epochs replaces."""

    def __init__(self, tensors, targets, on_chunk=None, on_batch=None, train_on_chunk=None, train_on_batch=None):
        self.tensors, self.targets, self.on_chunk, self.on_batch = tuple(tensors), targets, on_chunk, on_batch
        self.train_on_chunk, self.train_on_batch = train_on_chunk or on_chunk, train_on_batch or on_batch


class PointwiseDataset(Dataset):
    def __init__(self, file_or_frame, use_bce_loss=False):
        self.samples = file_or_frame if isinstance(file_or_frame, pd.DataFrame) else pd.read_csv(str(file_or_frame) + '.csv')
        self.use_bce_loss = use_bce_loss
        self.loss_fn = nn.BCEWithLogitsLoss(reduction='sum') if use_bce_loss else nn.MSELoss(reduction='sum')
        # column arrays once: the reference's per-sample DataFrame.iloc (base.py:25) is 14 ms per 512-batch
        self._u = self.samples['userId'].to_numpy()
        self._i = self.samples['movieId'].to_numpy()
        self._r = self.samples['rating'].to_numpy()

    def __getitem__(self, item):
        r = self._r[item]
        return self._u[item], self._i[item], r / 5.0 if self.use_bce_loss else r

    def __len__(self):
        return len(self.samples)

    def calculate_loss(self, y_pred, y_true):
        return self.loss_fn(y_pred, y_true.view(-1, 1).float())

    def get_graph(self, device):
        return None

    def use_collate(self):
        return None

    def resident_inputs(self, device=None, batch_size=None):
        """A ResidentInputs for datasets whose batch is a pure function of the sample rows (index ids), such that
        ``do_forward(model, batch, ...)`` over its batches equals the DataLoader loop; ``None`` (default): batches need the
        host collate (dense profiles).  eval_model uses it to skip the per-sample Python loop."""
        return None

    def _targets(self):
        r = self._r / 5.0 if self.use_bce_loss else self._r
        return torch.as_tensor(r, dtype=torch.float32)

    @staticmethod
    def do_forward(*args, **kwargs):
        raise NotImplementedError


def _first_rows(mask, limit=5):
    return np.flatnonzero(mask)[:limit].tolist()


class RankingDataset(Dataset):
    """Pair-wise samples (base.py:45-99): a DataFrame with ``userId``, ``positive_movieId``, ``negative_movieIds`` and
    ``negative_ratings`` (list-like per row), or the reference's ``<file>.h5`` (``pd.read_hdf``).  The negatives' lists are
    flattened once into a CSR with one row per sample (``_rowptr``, ``_neg_ids``, ``_neg_r``): the host ``__getitem__`` draws
    from it exactly as the reference draws from the frame, and the device-resident form (``resident_pairs``) uploads it once
    and draws with ``native.sample_negatives``.  Rows the reference cannot sample from are refused here, at construction."""

    def __init__(self, file_or_frame):
        self.samples = file_or_frame if isinstance(file_or_frame, pd.DataFrame) else pd.read_hdf(str(file_or_frame) + '.h5')
        self.loss_fn = BPR_loss
        self._w = 0.0            # w hyperparameter for dynamic negative sampling (base.py:55)
        self._resident = {}
        self._u = self.samples['userId'].to_numpy()
        self._pos = self.samples['positive_movieId'].to_numpy()
        ids = [np.asarray(x) for x in self.samples['negative_movieIds']]
        rts = [np.asarray(x) for x in self.samples['negative_ratings']]
        lens = np.fromiter((x.size for x in ids), dtype=np.int64, count=len(ids))
        rlens = np.fromiter((x.size for x in rts), dtype=np.int64, count=len(rts))
        if (lens == 0).any():
            raise ValueError(f"empty negative list in row(s) {_first_rows(lens == 0)}")
        if (lens != rlens).any():
            raise ValueError(f"negative_movieIds and negative_ratings differ in length in row(s) {_first_rows(lens != rlens)}")
        self._rowptr = np.zeros(len(ids) + 1, dtype=np.int64)
        np.cumsum(lens, out=self._rowptr[1:])
        self._neg_ids = np.concatenate(ids) if ids else np.zeros(0, dtype=np.int64)
        self._neg_r = np.concatenate(rts) if rts else np.zeros(0, dtype=np.float64)
        r = self._neg_r.astype(np.float64)
        row_of = np.repeat(np.arange(len(ids)), lens)
        bad = ~np.isfinite(r) | (r < 0)
        if bad.any():
            raise ValueError(f"negative, NaN or infinite negative rating in row(s) {np.unique(row_of[bad])[:5].tolist()}")
        if len(ids) and (np.maximum.reduceat(r, self._rowptr[:-1]) == 0).any():
            zero = np.maximum.reduceat(r, self._rowptr[:-1]) == 0
            raise ValueError(f"every negative rating is 0 in row(s) {_first_rows(zero)} (no distribution once w > 0)")

    @property
    def w(self):
        return self._w

    @w.setter
    def w(self, value):
        self._w = value           # the device CDF is rebuilt at the next draw (ResidentPairs.batch compares w)

    def _negative_sampling_probs(self, negative_ratings: np.ndarray, type='sum_dynamic'):
        if type == 'sum':
            probs = negative_ratings / sum(negative_ratings)
        elif type == 'sum_dynamic':
            negative_ratings_squared = negative_ratings ** self.w
            probs = negative_ratings_squared / sum(negative_ratings_squared)
        elif type == 'softmax':
            probs = softmax(torch.FloatTensor(negative_ratings), dim=0).numpy()
        else:
            probs = None    # uniform
        return probs

    def __getitem__(self, item):
        # the reference's draw (base.py:72-78) from the flattened rows: the same arrays, the same global numpy RNG calls
        s, e = self._rowptr[item], self._rowptr[item + 1]
        probs = self._negative_sampling_probs(np.array(self._neg_r[s:e]))
        negative = np.random.choice(self._neg_ids[s:e], p=probs)
        return self._u[item], self._pos[item], negative

    def __len__(self):
        return len(self.samples)

    def calculate_loss(self, out_pos, out_neg):
        return self.loss_fn(out_pos, out_neg)

    def get_graph(self, device):
        return None

    def use_collate(self):
        return None

    def resident_pairs(self, device=None):
        """A ResidentPairs when every batch is a function of the sample rows plus a negative drawn on the device (index ids);
        ``None`` (default): the DataLoader loop."""
        return None

    def _resident_pairs(self, device, users, positives, neg_positions):
        """Cached ResidentPairs over device tensors: user / positive positions (int64, sample order) and the negatives' positions
        (int32, the CSR's order)."""
        key = str(device)
        if key not in self._resident:
            rowptr = torch.from_numpy(self._rowptr).to(device)
            rating = torch.from_numpy(self._neg_r.astype(np.float32)).to(device)
            self._resident[key] = ResidentPairs(self, users, positives, NegativeSampler(rowptr, neg_positions, rating))
        return self._resident[key]

    @staticmethod
    def do_forward(*args, **kwargs):
        raise NotImplementedError


class NegativeSampler:
    """The negatives' CSR on the device and its CDF for the current ``w`` (native.negative_cdf, rebuilt when w changes); ``draw``
    is one native.sample_negatives call.  ``flag`` is set by a row without a distribution (checked by ``check``)."""

    def __init__(self, rowptr, neg, rating):
        self.rowptr, self.neg, self.rating = rowptr, neg.to(torch.int32).contiguous(), rating
        self.cdf = torch.empty_like(rating)
        self.flag = torch.zeros(1, dtype=torch.int32, device=rating.device)
        self.cdf_w = None

    def draw(self, pick, w, seed, slot0):
        from ... import native
        if self.cdf_w is None or self.cdf_w != w:
            native.negative_cdf(self.rowptr, self.rating, float(w), out=self.cdf, flag=self.flag)
            self.cdf_w = w
        return native.sample_negatives(self.rowptr, self.cdf, self.neg, pick, seed, slot0)

    def check(self):
        """Synchronising: ValueError for a row without a distribution since the last check, IndexError (native.check_oob) for
        an out-of-range pick or position."""
        from ... import native
        if int(self.flag.item()) != 0:
            self.flag.zero_()
            raise ValueError(f"a negative row has no finite positive total of rating ** w at w = {self.cdf_w}")
        native.check_oob(self.rating.device)


class ResidentPairs:
    """Pair-wise training inputs resident on the device: ``batch(pick, seed, slot0)`` gathers the picked samples' user and positive
    positions and draws one negative each (slot slot0 + b for the b-th pick) — the tuple the dataset's ``do_forward`` takes."""

    def __init__(self, dataset, users, positives, sampler):
        self.dataset, self.users, self.positives, self.sampler = dataset, users, positives, sampler

    def __len__(self):
        return self.users.numel()

    def batch(self, pick, seed, slot0):
        pick = pick.contiguous()
        return self.users[pick], self.positives[pick], self.sampler.draw(pick, self.dataset.w, seed, slot0)

    def check(self):
        self.sampler.check()


def BPR_loss(out_pos, out_neg):
    return torch.sum(-torch.log(torch.sigmoid(out_pos - out_neg)))
