"""Baselines the reference's evaluation compares the NCF models with.  ``KernelMF`` is its collaborative-filtering baseline
(cf_baseline.py: the matrix_factorization package's KernelMF with the linear kernel): biased matrix factorisation

    r^ = mu + b_u + b_i + p_u . q_i

fitted by per-sample SGD.  Here the fit runs on the device as stratified SGD (csrc/kmf.hip, THE CONTRACT in include/ncf_abi.h): the
rating matrix is cut into W x W blocks, the W blocks of a stratum share no user and no item and run side by side, and a fit is a
fixed function of its inputs, W included.  There is no host path."""
import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import native

ROW_ALIGN = 32      # floats: a table row starts on a 128-byte line, so no line holds rows of two blocks


def _positions(t, what, n=None):
    if not torch.is_tensor(t) or t.dtype != torch.int64 or t.dim() != 1:
        raise ValueError(f"KernelMF: {what} must be a 1-D int64 tensor of positions")
    if n is not None and t.numel() != n:
        raise ValueError(f"KernelMF: {what} has {t.numel()} entries, expected {n}")


def _deal_blocks(ids, count, W):
    """Ids to W blocks, round-robin in descending order of their number of ratings (stable: ties go by position), so every block gets
    its share of the heavy rows and block sizes differ by at most one id."""
    counts = torch.bincount(ids, minlength=count)
    order = torch.argsort(-counts, stable=True)
    block = torch.empty(count, dtype=torch.int32, device=ids.device)
    block[order] = (torch.arange(count, device=ids.device) % W).to(torch.int32)
    return block, counts


class KernelMF:
    """``KernelMF(...).fit(user_pos, item_pos, rating, num_users, num_items)``; then ``predict``, ``as_mf()`` (the project's MF module
    with the baseline's tables: every ranking and evaluation function takes it) and ``update_users`` (fold-in of new ratings).

    ``n_blocks`` (W) defaults to min(CU count, num_users, num_items).  It decides the order of the updates and hence the bits of the
    fit, so the value used is kept in ``n_blocks_``."""

    def __init__(self, n_factors=100, n_epochs=100, lr=0.01, reg=1.0, init_mean=0.0, init_sd=0.1, min_rating=0.0, max_rating=5.0,
                 n_blocks=None):
        if not isinstance(n_factors, (int, np.integer)) or not 1 <= n_factors <= native.KMF_MAX_FACTORS:
            raise ValueError(f"KernelMF: n_factors = {n_factors!r} (an integer in 1 .. {native.KMF_MAX_FACTORS})")
        if not isinstance(n_epochs, (int, np.integer)) or n_epochs < 0:
            raise ValueError(f"KernelMF: n_epochs = {n_epochs!r}")
        for name, v in (("lr", lr), ("reg", reg), ("init_mean", init_mean), ("init_sd", init_sd), ("min_rating", min_rating),
                        ("max_rating", max_rating)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
                raise ValueError(f"KernelMF: {name} = {v!r} is not a finite number")
        if lr <= 0 or reg < 0 or init_sd < 0 or not min_rating < max_rating:
            raise ValueError(f"KernelMF: lr > 0, reg >= 0, init_sd >= 0 and min_rating < max_rating (got {lr}, {reg}, {init_sd}, "
                             f"{min_rating}, {max_rating})")
        if n_blocks is not None and (not isinstance(n_blocks, (int, np.integer)) or not 1 <= n_blocks <= native.KMF_MAX_BLOCKS):
            raise ValueError(f"KernelMF: n_blocks = {n_blocks!r} (None or an integer in 1 .. {native.KMF_MAX_BLOCKS})")
        self.n_factors, self.n_epochs, self.lr, self.reg = int(n_factors), int(n_epochs), float(lr), float(reg)
        self.init_mean, self.init_sd, self.min_rating, self.max_rating = float(init_mean), float(init_sd), float(min_rating), float(max_rating)
        self.n_blocks = None if n_blocks is None else int(n_blocks)
        self.user_table_ = self.item_table_ = None      # (U, ld) / (I, ld) fp32: F factors, the bias, padding
        self.global_mean_ = None                        # mu, an fp32 value
        self.n_blocks_ = None
        self.train_rmse_ = []
        self._mf = None

    # ------------------------------------------------------------------ fit
    def build_plan(self, user_pos, item_pos, rating, num_users, num_items, W):
        """The plan of a fit, on the samples' device: users and items dealt to W blocks, samples ordered stratum-major by a stable
        sort on s * W + a (a the user's block, s = (item's block - a) mod W), so input order survives within a block."""
        ub, ucount = _deal_blocks(user_pos, num_users, W)
        ib, icount = _deal_blocks(item_pos, num_items, W)
        a, b = ub[user_pos].to(torch.int64), ib[item_pos].to(torch.int64)
        key = torch.remainder(b - a, W) * W + a
        order = torch.argsort(key, stable=True)
        ptr = torch.zeros(W * W + 1, dtype=torch.int64, device=key.device)
        ptr[1:] = torch.cumsum(torch.bincount(key, minlength=W * W), 0)
        return {"W": W, "user": user_pos[order].to(torch.int32), "item": item_pos[order].to(torch.int32), "rating": rating[order].contiguous(),
                "block_ptr": ptr, "user_block": ub, "item_block": ib, "user_count": ucount, "item_count": icount}

    def fit(self, user_pos, item_pos, rating, num_users, num_items, generator: Optional[torch.Generator] = None, epoch_callback=None,
            at_epochs: Sequence[int] = ()):
        """Fits on int64 positions and fp32 ratings that live on the GPU.  mu is the float64 mean of the ratings rounded to fp32;
        the factors are N(init_mean, init_sd) from ``generator`` (one normal_ draw of (num_users, F), then one of (num_items, F), on
        the generator's device), the biases start at 0, and rows without any rating are zero, bias included: such an id predicts mu
        plus the known side's bias.  With ``at_epochs`` (increasing, within 1 .. n_epochs) the fit stops after those epochs and calls
        ``epoch_callback(self, epoch)`` with the model usable as it then stands: the first k epochs of a fit ARE the k-epoch fit.
        ``train_rmse_[e]`` is sqrt(sum of the epoch's squared errors / n), each error taken before its update."""
        n = user_pos.numel() if torch.is_tensor(user_pos) else None
        _positions(user_pos, "user_pos")
        _positions(item_pos, "item_pos", n)
        if not torch.is_tensor(rating) or rating.dtype != torch.float32 or rating.dim() != 1 or rating.numel() != n:
            raise ValueError(f"KernelMF: rating must be a 1-D float32 tensor of {n} entries")
        num_users, num_items = int(num_users), int(num_items)
        if n == 0 or num_users < 1 or num_items < 1:
            raise ValueError(f"KernelMF: nothing to fit ({n} ratings, {num_users} users, {num_items} items)")
        stops = [int(e) for e in at_epochs]
        if any(b <= a for a, b in zip([0] + stops, stops)) or (stops and stops[-1] > self.n_epochs):
            raise ValueError(f"KernelMF: at_epochs = {tuple(at_epochs)!r} must increase within 1 .. n_epochs = {self.n_epochs}")
        if stops and epoch_callback is None:
            raise ValueError("KernelMF: at_epochs without an epoch_callback")
        dev = user_pos.device
        if dev.type != "cuda" or item_pos.device != dev or rating.device != dev:
            raise RuntimeError(f"KernelMF.fit runs on the GPU: the samples must live on one GPU (got {dev}, {item_pos.device}, {rating.device}); "
                               "there is no CPU path")
        W = self.n_blocks
        if W is None:
            W = min(torch.cuda.get_device_properties(dev).multi_processor_count, num_users, num_items, native.KMF_MAX_BLOCKS)
        F = self.n_factors
        ld = (F + 1 + ROW_ALIGN - 1) // ROW_ALIGN * ROW_ALIGN
        plan = self.build_plan(user_pos, item_pos, rating, num_users, num_items, W)
        self.global_mean_ = float(np.float32(float(rating.to(torch.float64).sum().item()) / n))
        tables = []
        for rows, count in ((num_users, plan["user_count"]), (num_items, plan["item_count"])):
            gdev = generator.device if generator is not None else dev
            fac = torch.empty((rows, F), dtype=torch.float32, device=gdev).normal_(self.init_mean, self.init_sd, generator=generator)
            t = torch.zeros((rows, ld), dtype=torch.float32, device=dev)
            t[:, :F] = fac.to(dev)
            t[count == 0] = 0.0
            tables.append(t)
        self.user_table_, self.item_table_ = tables
        self.n_blocks_, self.num_users_, self.num_items_, self.n_samples_ = W, num_users, num_items, n
        self._sse = torch.zeros((self.n_epochs, W), dtype=torch.float64, device=dev)
        self.train_rmse_, self._mf = [], None
        done = 0
        for stop in stops + ([self.n_epochs] if not stops or stops[-1] < self.n_epochs else []):
            native.kmf_epoch(self.user_table_, self.item_table_, F, plan["user"], plan["item"], plan["rating"], plan["block_ptr"],
                             plan["user_block"], plan["item_block"], self.global_mean_, self.lr, self.reg, stop - done,
                             sse=self._sse[done:stop])
            done = stop
            if stop in stops:
                self._finish(done)
                epoch_callback(self, stop)
        self._finish(done)
        return self

    def _finish(self, done):
        """Synchronises: the flag word, and the per-epoch loss summed over the W partials in index order, in float64."""
        self.check()
        self._mf = None
        sse = self._sse[:done].cpu().numpy()
        self.train_rmse_ = []
        for row in sse:
            acc = 0.0
            for v in row:
                acc = acc + float(v)
            self.train_rmse_.append(math.sqrt(acc / self.n_samples_))

    def check(self):
        """Raises IndexError when a kernel of this device met what it refuses (an id outside its table, a sample in the wrong block,
        a broken pointer); such samples were skipped."""
        self._fitted()
        native.check_kmf(self.user_table_.device)

    def _fitted(self):
        if self.user_table_ is None:
            raise RuntimeError("KernelMF: not fitted")

    def fit_dataset(self, dataset, device="cuda", **fit_args):
        """fit on the positions and ratings of a FixedPointwiseDataset over an index provider (its ``resident_inputs()``)."""
        dev = torch.device(device)
        res = dataset.resident_inputs(dev)
        if res is None:
            raise ValueError("KernelMF.fit_dataset: the dataset's provider hands out dense rows, not positions")
        u, i = (t.to(dev) for t in res.tensors)
        if res.on_chunk is not None:
            u, i = res.on_chunk(u, i)
        cp = dataset.content_provider
        return self.fit(u.contiguous(), i.contiguous(), res.targets.to(dev), cp.get_num_users(), cp.get_num_items(), **fit_args)

    # ------------------------------------------------------------------ fold-in
    def update_users(self, rowptr, col, rating, user_pos, n_epochs: Optional[int] = None, lr: Optional[float] = None):
        """The package's update_users: ``n_epochs`` SGD passes (default: the model's) over the ratings of the users ``user_pos``
        (int64 positions, no user twice) against the FIXED item table; row k of the CSR (``rowptr`` int64, ``col`` int32 item
        positions, ``rating`` fp32) holds user_pos[k]'s ratings.  Rows continue from where they stand (a user without training
        ratings from zero).  Returns the (n_epochs, n_users) float64 sums of squared errors."""
        self._fitted()
        _positions(user_pos, "user_pos")
        n_epochs = self.n_epochs if n_epochs is None else int(n_epochs)
        lr = self.lr if lr is None else float(lr)
        if n_epochs < 0 or not math.isfinite(lr) or lr <= 0:
            raise ValueError(f"KernelMF.update_users: n_epochs = {n_epochs}, lr = {lr}")
        if torch.unique(user_pos).numel() != user_pos.numel():
            raise ValueError("KernelMF.update_users: a user is listed twice")
        sse = native.kmf_fold_users(self.user_table_, self.item_table_, self.n_factors, user_pos.to(torch.int32), rowptr, col, rating,
                                    self.global_mean_, lr, self.reg, n_epochs)
        self._mf = None
        self.check()
        return sse

    # ------------------------------------------------------------------ scoring
    def as_mf(self):
        """The project's MF module computing this model: user table [p_u, b_u + mu, 1], item table [q_i, 1, b_i] of width F + 2,
        zero Linear biases, frozen and in eval mode, on the fit's device.  top_k_items, rank_of_items, eval_full_ranking, eval_model
        and [state_dict, kwargs] checkpoints work on it as on any MF."""
        self._fitted()
        if self._mf is None:
            from .neural_collaborative_filtering.models.mf import MF
            F, pu, qi = self.n_factors, self.user_table_, self.item_table_
            one_u, one_i = pu.new_ones((pu.shape[0], 1)), qi.new_ones((qi.shape[0], 1))
            mu = torch.tensor(self.global_mean_, dtype=torch.float32, device=pu.device)
            ut = torch.cat([pu[:, :F], (pu[:, F] + mu)[:, None], one_u], 1).contiguous()
            it = torch.cat([qi[:, :F], one_i, qi[:, F:F + 1]], 1).contiguous()
            mf = MF(item_dim=qi.shape[0], user_dim=pu.shape[0], item_emb=F + 2, user_emb=F + 2).to(pu.device)
            with torch.no_grad():
                for lin, tab in ((mf.user_embeddings[0], ut), (mf.item_embeddings[0], it)):
                    lin.weight = torch.nn.Parameter(tab.t(), requires_grad=False)      # id-major, as row_major_embedding_ lays it
                    lin.bias.zero_()
            self._mf = mf.requires_grad_(False).eval()
        return self._mf

    def predict(self, user_pos, item_pos, clip=True):
        """(n,) predictions for int64 positions on the fit's device: as_mf()'s forward, clamped to [min_rating, max_rating] when
        ``clip`` is set."""
        _positions(user_pos, "user_pos")
        _positions(item_pos, "item_pos", user_pos.numel())
        with torch.no_grad():
            out = self.as_mf()(user_pos.contiguous(), item_pos.contiguous()).view(-1)
        return out.clamp(self.min_rating, self.max_rating) if clip else out
