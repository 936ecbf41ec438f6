"""Baselines the reference's evaluation compares the NCF models with.  ``KernelMF`` is its collaborative-filtering baseline
(cf_baseline.py: the matrix_factorization package's KernelMF with the linear kernel): biased matrix factorisation

    r^ = mu + b_u + b_i + p_u . q_i

fitted by per-sample SGD.  Here the fit runs on the device as stratified SGD (csrc/kmf.hip, THE CONTRACT in include/ncf_abi.h): the
rating matrix is cut into W x W blocks, the W blocks of a stratum share no user and no item and run side by side, and a fit is a
fixed function of its inputs, W included.  There is no host path.

``ItemKNN`` is the neighbourhood baseline such comparisons are also read against (Sarwar et al. 2001; Surprise KNNBasic, LensKit
ItemItem): shrunk cosine similarities of the items over the rating matrix, each item's k nearest neighbours, scores from the
neighbours a user rated (csrc/knn.hip, THE CONTRACT in include/ncf_abi.h).  Its neighbour table is also "more like this item".

``ImplicitALS`` is the implicit-feedback baseline a full-catalogue top-K number is usually asked to beat (Hu, Koren & Volinsky 2008;
implicit's AlternatingLeastSquares; the iALS of Rendle et al. 2021): every stored entry is a preference of 1 held with confidence
1 + alpha * value, every other pair a preference of 0 with confidence 1, and the two factor tables are solved in turn, each row by
one Cholesky factorisation on the device (csrc/als.hip, THE CONTRACT in include/ncf_abi.h).  A new user is folded in exactly, by one
such solve against the fixed item table.

``EASE`` is the closed-form item-item baseline that most often wins that comparison (Steck 2019, "Embarrassingly Shallow Autoencoders
for Sparse Data"): W = the off-diagonal of (X^T X + reg 1)^-1 with every column divided by minus its diagonal entry, scores X W.  No
epochs, no seeds, one hyper-parameter; the Gram matrix, its inversion (a blocked Gauss-Jordan elimination whose updates are fp32
MFMA GEMMs), the weights and the scores all run on the device (csrc/ease.hip, THE CONTRACT in include/ncf_abi.h).

``SLIM`` is the model EASE is measured against in its own paper (Ning & Karypis 2011, "SLIM: Sparse Linear Methods for Top-N
Recommender Systems"): the same item-item regression X ~ X W with diag(W) = 0, solved under an L1 + L2 penalty (and W >= 0) instead
of in closed form, which makes W sparse.  Every column is one cyclic coordinate descent on EASE's Gram matrix, one workgroup per
column, with the bits of the serial loop (csrc/slim.hip, THE CONTRACT in include/ncf_abi.h); the weights are served by EASE's scorer."""
import math
import numbers
from types import SimpleNamespace
from typing import Optional, Sequence

import numpy as np
import torch

from . import native
from .native import _finite, _int_in      # the scalar checks of the bindings: a bool is no integer and no number

ROW_ALIGN = 32      # floats: a table row starts on a 128-byte line, so no line holds rows of two blocks
INT_MAX = 2 ** 31 - 1


def _positions(who, t, what, n=None):
    if not torch.is_tensor(t) or t.dtype != torch.int64 or t.dim() != 1:
        raise ValueError(f"{who}: {what} must be a 1-D int64 tensor of positions")
    if n is not None and t.numel() != n:
        raise ValueError(f"{who}: {what} has {t.numel()} entries, expected {n}")


def _one_gpu(who, what, *tensors):
    """The device of tensors a fit reads, which must be one GPU."""
    devs = [t.device for t in tensors]
    if devs[0].type != "cuda" or any(d != devs[0] for d in devs):
        raise RuntimeError(f"{who} runs on the GPU: the {what} must live on one GPU (got {', '.join(str(d) for d in devs)}); "
                           "there is no CPU path")
    return devs[0]


def _ratings_csr(who, ratings):
    """A ratings CSR argument: a SparseRatings-like object (rowptr / col / val) or a (rowptr, col, val) tuple, as the kernels take it."""
    if isinstance(ratings, (tuple, list)) and len(ratings) == 3:
        rowptr, col, val = ratings
    elif all(hasattr(ratings, a) for a in ("rowptr", "col", "val")):
        if getattr(ratings, "pair_row", None) is not None:
            raise ValueError(f"{who}: the ratings share rows through pair_row; pass the CSR with one row per user")
        rowptr, col, val = ratings.rowptr, ratings.col, ratings.val
    else:
        raise ValueError(f"{who}: ratings must be a SparseRatings or a (rowptr, col, val) tuple")
    for t, what in ((rowptr, "rowptr"), (col, "col"), (val, "val")):
        if not torch.is_tensor(t) or t.dim() != 1:
            raise ValueError(f"{who}: {what} must be a 1-D tensor")
    if rowptr.dtype not in (torch.int64, torch.int32) or col.dtype not in (torch.int64, torch.int32) or val.dtype != torch.float32:
        raise ValueError(f"{who}: rowptr / col must be integer tensors and val float32")
    if rowptr.numel() < 1 or col.numel() != val.numel():
        raise ValueError(f"{who}: rowptr is empty or col and val differ in length")
    return rowptr.to(torch.int64).contiguous(), col.to(torch.int32).contiguous(), val.contiguous()


def _mf_of_tables(user_table, item_table):
    """The project's MF module over two (rows, F) fp32 tables: zero Linear biases, frozen and in eval mode, on the tables' device."""
    from .neural_collaborative_filtering.models.mf import MF
    F = user_table.shape[1]
    mf = MF(item_dim=item_table.shape[0], user_dim=user_table.shape[0], item_emb=F, user_emb=F).to(user_table.device)
    with torch.no_grad():
        for lin, tab in ((mf.user_embeddings[0], user_table), (mf.item_embeddings[0], item_table)):
            lin.weight = torch.nn.Parameter(tab.contiguous().t(), requires_grad=False)      # id-major, as row_major_embedding_ lays it
            lin.bias.zero_()
    return mf.requires_grad_(False).eval()


class _Baseline:
    """The fit front end of the baselines: the checks of the samples or of the CSR a fit is given, and fit_dataset.  Every
    message names the concrete class."""

    def _samples(self, user_pos, item_pos, rating, num_users, num_items):
        """Checks the samples of ``fit`` — int64 positions and fp32 ratings of one length, something to fit, all on one GPU — and
        returns ``(n, num_users, num_items, device)``."""
        who = type(self).__name__
        _positions(who, user_pos, "user_pos")
        n = user_pos.numel()
        _positions(who, item_pos, "item_pos", n)
        if not torch.is_tensor(rating) or rating.dtype != torch.float32 or rating.dim() != 1 or rating.numel() != n:
            raise ValueError(f"{who}: rating must be a 1-D float32 tensor of {n} entries")
        num_users, num_items = int(num_users), int(num_items)
        if n == 0 or num_users < 1 or num_items < 1:
            raise ValueError(f"{who}: nothing to fit ({n} ratings, {num_users} users, {num_items} items)")
        return n, num_users, num_items, _one_gpu(f"{who}.fit", "samples", user_pos, item_pos, rating)

    def _csr(self, rowptr, col, val, num_items):
        """Checks the user CSR of ``fit_csr`` — _ratings_csr's, something to fit, all on one GPU — and returns ``(rowptr int64, col int32,
        val, num_items, device)``."""
        who = type(self).__name__
        rowptr, col, val = _ratings_csr(f"{who}.fit_csr", (rowptr, col, val))
        I = int(num_items)
        if I < 1 or rowptr.numel() < 2 or col.numel() == 0:
            raise ValueError(f"{who}: nothing to fit ({col.numel()} ratings, {rowptr.numel() - 1} users, {I} items)")
        return rowptr, col, val, I, _one_gpu(f"{who}.fit_csr", "CSR", rowptr, col, val)

    def fit_dataset(self, dataset, device="cuda", **fit_args):
        """fit on the positions and ratings of a FixedPointwiseDataset over an index provider (its ``resident_inputs()``)."""
        dev = torch.device(device)
        res = dataset.resident_inputs(dev)
        if res is None:
            raise ValueError(f"{type(self).__name__}.fit_dataset: the dataset's provider hands out dense rows, not positions")
        u, i = (t.to(dev) for t in res.tensors)
        if res.on_chunk is not None:
            u, i = res.on_chunk(u, i)
        cp = dataset.content_provider
        return self.fit(u.contiguous(), i.contiguous(), res.targets.to(dev), cp.get_num_users(), cp.get_num_items(), **fit_args)


def _deal_blocks(ids, count, W):
    """Ids to W blocks, round-robin in descending order of their number of ratings (stable: ties go by position), so every block gets
    its share of the heavy rows and block sizes differ by at most one id."""
    counts = torch.bincount(ids, minlength=count)
    order = torch.argsort(-counts, stable=True)
    block = torch.empty(count, dtype=torch.int32, device=ids.device)
    block[order] = (torch.arange(count, device=ids.device) % W).to(torch.int32)
    return block, counts


class KernelMF(_Baseline):
    """``KernelMF(...).fit(user_pos, item_pos, rating, num_users, num_items)``; then ``predict``, ``as_mf()`` (the project's MF module
    with the baseline's tables: every ranking and evaluation function takes it) and ``update_users`` (fold-in of new ratings).

    ``n_blocks`` (W) defaults to min(CU count, num_users, num_items).  It decides the order of the updates and hence the bits of the
    fit, so the value used is kept in ``n_blocks_``."""

    def __init__(self, n_factors=100, n_epochs=100, lr=0.01, reg=1.0, init_mean=0.0, init_sd=0.1, min_rating=0.0, max_rating=5.0,
                 n_blocks=None):
        who = "KernelMF"
        self.n_factors = _int_in(who, n_factors, "n_factors", 1, native.KMF_MAX_FACTORS)
        self.n_epochs = _int_in(who, n_epochs, "n_epochs", 0, INT_MAX)
        self.lr, self.reg, self.init_sd = _finite(who, lr, "lr", 0.0), _finite(who, reg, "reg", 0.0), _finite(who, init_sd, "init_sd", 0.0)
        self.init_mean = _finite(who, init_mean, "init_mean")
        self.min_rating, self.max_rating = _finite(who, min_rating, "min_rating"), _finite(who, max_rating, "max_rating")
        if not self.lr > 0 or not self.min_rating < self.max_rating:
            raise ValueError(f"{who}: lr > 0 and min_rating < max_rating (got {lr}, {min_rating}, {max_rating})")
        self.n_blocks = None if n_blocks is None else _int_in(who, n_blocks, "n_blocks", 1, native.KMF_MAX_BLOCKS)
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
        stops = [int(e) for e in at_epochs]
        if any(b <= a for a, b in zip([0] + stops, stops)) or (stops and stops[-1] > self.n_epochs):
            raise ValueError(f"KernelMF: at_epochs = {tuple(at_epochs)!r} must increase within 1 .. n_epochs = {self.n_epochs}")
        if stops and epoch_callback is None:
            raise ValueError("KernelMF: at_epochs without an epoch_callback")
        n, num_users, num_items, dev = self._samples(user_pos, item_pos, rating, num_users, num_items)
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

    # ------------------------------------------------------------------ fold-in
    def update_users(self, rowptr, col, rating, user_pos, n_epochs: Optional[int] = None, lr: Optional[float] = None):
        """The package's update_users: ``n_epochs`` SGD passes (default: the model's) over the ratings of the users ``user_pos``
        (int64 positions, no user twice) against the FIXED item table; row k of the CSR (``rowptr`` int64, ``col`` int32 item
        positions, ``rating`` fp32) holds user_pos[k]'s ratings.  Rows continue from where they stand (a user without training
        ratings from zero).  Returns the (n_epochs, n_users) float64 sums of squared errors."""
        self._fitted()
        _positions("KernelMF.update_users", user_pos, "user_pos")
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
            F, pu, qi = self.n_factors, self.user_table_, self.item_table_
            one_u, one_i = pu.new_ones((pu.shape[0], 1)), qi.new_ones((qi.shape[0], 1))
            mu = torch.tensor(self.global_mean_, dtype=torch.float32, device=pu.device)
            self._mf = _mf_of_tables(torch.cat([pu[:, :F], (pu[:, F] + mu)[:, None], one_u], 1),
                                     torch.cat([qi[:, :F], one_i, qi[:, F:F + 1]], 1))
        return self._mf

    def predict(self, user_pos, item_pos, clip=True):
        """(n,) predictions for int64 positions on the fit's device: as_mf()'s forward, clamped to [min_rating, max_rating] when
        ``clip`` is set."""
        _positions("KernelMF.predict", user_pos, "user_pos")
        _positions("KernelMF.predict", item_pos, "item_pos", user_pos.numel())
        with torch.no_grad():
            out = self.as_mf()(user_pos.contiguous(), item_pos.contiguous()).view(-1)
        return out.clamp(self.min_rating, self.max_rating) if clip else out


# ---------------------------------------------------------------------------------------- ItemKNN
def build_transpose(rowptr, col, val, num_items):
    """``(colptr (I + 1) int64, row int32, tval fp32)``: the CSR by item, torch ops on whatever device the CSR is on.  A stable
    sort of the entries on their column keeps the users of a column in ascending order."""
    counts = rowptr[1:] - rowptr[:-1]
    users = torch.repeat_interleave(torch.arange(counts.numel(), device=col.device), counts)
    c64 = col.to(torch.int64)
    order = torch.argsort(c64, stable=True)
    colptr = torch.zeros(num_items + 1, dtype=torch.int64, device=col.device)
    inside = c64[(c64 >= 0) & (c64 < num_items)]           # an id outside the items is the kernels' to flag, not bincount's to index
    colptr[1:] = torch.cumsum(torch.bincount(inside, minlength=num_items), 0)
    keep = order[(c64[order] >= 0) & (c64[order] < num_items)]
    return colptr, users[keep].to(torch.int32), val[keep].contiguous()


def build_csr(user_pos, item_pos, rating, num_users, num_items):
    """``(rowptr (U + 1) int64, col int32, val fp32)`` of samples in any order: torch ops on the samples' device."""
    order = torch.argsort(user_pos * num_items + item_pos, stable=True)
    rowptr = torch.zeros(num_users + 1, dtype=torch.int64, device=user_pos.device)
    rowptr[1:] = torch.cumsum(torch.bincount(user_pos, minlength=num_users), 0)
    return rowptr, item_pos[order].to(torch.int32), rating[order].contiguous()


class ItemKNN(_Baseline):
    """Item-item k-nearest-neighbours over the rating matrix (csrc/knn.hip, THE CONTRACT in include/ncf_abi.h): shrunk cosine
    similarities ``s_ij = cos(i, j) * co / (co + shrink)`` of items co-rated by at least ``min_support`` users, the ``k`` largest
    positive ones kept per item, and scores ``sum s_ij * v_uj`` over the neighbours a user rated, divided by ``sum s_ij`` with
    ``weighted_average`` (``fill`` where no neighbour was rated).  ``fit`` / ``fit_dataset`` / ``fit_csr``; then ``neighbours``,
    ``similar_items``, ``scores``, ``predict``; ``recommend.item_knn_top_k`` / ``item_knn_ranks`` rank with it.  A fit is a fixed
    function of its inputs, bit for bit.  There is no host path."""

    def __init__(self, k=50, shrink=0.0, min_support=1, weighted_average=True, fill=0.0):
        who = "ItemKNN"
        self.k = _int_in(who, k, "k", 1, native.KNN_MAX_N)
        self.min_support = _int_in(who, min_support, "min_support", 1, INT_MAX)
        self.shrink, self.fill = _finite(who, shrink, "shrink", 0.0), _finite(who, fill, "fill")
        if not isinstance(weighted_average, (bool, np.bool_)):
            raise ValueError(f"{who}: weighted_average = {weighted_average!r} is not a bool")
        self.weighted_average = bool(weighted_average)
        self.nb_pos_ = self.nb_sim_ = self.nb_cnt_ = None      # (I, k) int32 / (I, k) fp32 / (I,) int32
        self.item_sq_ = None                                   # (I,) fp32 squared norms
        self.num_items_ = None

    # ------------------------------------------------------------------ fit
    build_transpose = staticmethod(build_transpose)

    def fit_csr(self, rowptr, col, val, num_items, block_bytes: int = 256 << 20, col_tile: int = 0):
        """Fits on a user CSR on the GPU: ``rowptr`` (U + 1) int64, ``col`` int32 item positions strictly ascending inside a row,
        ``val`` fp32 (SparseRatings' arrays as they are).  The similarity rows are computed ``block_bytes`` at a time and the table
        selected from each block by native.topk_rows; the table does not depend on the blocking.  Synchronises once, in check()."""
        rowptr, col, val, I, dev = self._csr(rowptr, col, val, num_items)
        colptr, row, tval = self.build_transpose(rowptr, col, val, I)
        sq = native.knn_item_sq(colptr, tval)
        N = self.k
        pos = torch.empty((I, N), dtype=torch.int32, device=dev)
        sim = torch.empty((I, N), dtype=torch.float32, device=dev)
        cnt = torch.empty(I, dtype=torch.int32, device=dev)
        rows = max(1, min(native.KNN_MAX_ROWS, int(block_bytes) // (4 * I)))
        for i0 in range(0, I, rows):
            i1 = min(I, i0 + rows)
            block = native.knn_sim_rows(rowptr, col, val, colptr, row, tval, sq, (i0, i1), self.min_support, self.shrink, col_tile)
            s, idx, _ = native.topk_rows(block, N)
            live = (idx >= 0) & (s > 0)                          # a selected zero is no neighbour; the live slots are a prefix
            pos[i0:i1] = torch.where(live, idx, torch.full_like(idx, -1))
            sim[i0:i1] = torch.where(live, s, torch.zeros_like(s))
            cnt[i0:i1] = live.sum(1).to(torch.int32)
        self.nb_pos_, self.nb_sim_, self.nb_cnt_, self.item_sq_, self.num_items_ = pos, sim, cnt, sq, I
        self.check()
        return self

    def fit(self, user_pos, item_pos, rating, num_users, num_items, **fit_args):
        """Fits on int64 positions and fp32 ratings that live on the GPU (KernelMF.fit's arguments): the CSR is built on the device by
        a stable sort on (user, item).  A (user, item) pair given twice raises in check()."""
        _, num_users, num_items, _ = self._samples(user_pos, item_pos, rating, num_users, num_items)
        rowptr, col, val = self.build_csr(user_pos, item_pos, rating, num_users, num_items)
        return self.fit_csr(rowptr, col, val, num_items, **fit_args)

    build_csr = staticmethod(build_csr)

    def check(self):
        """Synchronises.  Raises ValueError when a fit walked a row whose columns do not strictly ascend, and IndexError when a kernel
        of this device met an id outside its range; each raises once and is then cleared."""
        self._fitted()
        dev = self.nb_pos_.device
        native.check_knn(dev)
        native.check_oob(dev)

    def _fitted(self):
        if self.nb_pos_ is None:
            raise RuntimeError("ItemKNN: not fitted")

    # ------------------------------------------------------------------ the table
    @property
    def neighbours(self):
        """``(nb_sim (I, k) fp32, nb_pos (I, k) int64, nb_cnt (I,) int32)``: each item's neighbours by falling similarity, ties to the
        lower position; past the count the similarity is 0 and the position -1."""
        self._fitted()
        return self.nb_sim_, self.nb_pos_.to(torch.int64), self.nb_cnt_

    def similar_items(self, item_pos, k: Optional[int] = None):
        """"More like this": ``(scores (n, k) fp32, item_positions (n, k) int64, counts (n,) int32)`` of the listed items' nearest
        neighbours, in ``top_k_items``' form (past the count: score -inf, position -1).  ``k`` defaults to the table's width."""
        self._fitted()
        k = self.k if k is None else k
        k = _int_in("ItemKNN.similar_items", k, "k", 1, self.k)
        _positions("ItemKNN.similar_items", item_pos, "item_pos")
        pos = self.nb_pos_[item_pos, :k].to(torch.int64)
        sim = self.nb_sim_[item_pos, :k]
        return torch.where(pos >= 0, sim, torch.full_like(sim, float("-inf"))), pos, self.nb_cnt_[item_pos].clamp_max(k)

    # ------------------------------------------------------------------ scoring
    def scores(self, ratings, user_rows, item_range=None, stage_cap: int = 0):
        """(B, i1 - i0) fp32 scores of the rows ``user_rows`` (int64) of ``ratings`` — a SparseRatings or a (rowptr, col, val) tuple
        over the fitted items, not necessarily the fitted ratings, so new users work — against the items ``item_range`` = (i0, i1)
        (default: all)."""
        self._fitted()
        rowptr, col, val = _ratings_csr("ItemKNN.scores", ratings)
        return native.knn_scores(rowptr, col, val, user_rows.contiguous() if torch.is_tensor(user_rows) else user_rows, self.nb_pos_,
                                 self.nb_sim_, self.nb_cnt_, item_range, self.weighted_average, self.fill, stage_cap)

    def predict(self, ratings, user_rows, item_pos, clip=None):
        """(n,) fp32 scores of the pairs (row ``user_rows[k]`` of ``ratings``, item ``item_pos[k]``), int64 both: ``scores``' values
        bit for bit, clamped to ``clip`` = (lo, hi) when given."""
        self._fitted()
        rowptr, col, val = _ratings_csr("ItemKNN.predict", ratings)
        if clip is not None and (len(clip) != 2 or not clip[0] < clip[1]):
            raise ValueError(f"ItemKNN.predict: clip = {clip!r} (None or (lo, hi) with lo < hi)")
        out = native.knn_predict(rowptr, col, val, user_rows, item_pos, self.nb_pos_, self.nb_sim_, self.nb_cnt_, self.weighted_average,
                                 self.fill)
        return out if clip is None else out.clamp(float(clip[0]), float(clip[1]))


# ---------------------------------------------------------------------------------------- ImplicitALS
class ImplicitALS(_Baseline):
    """Implicit-feedback ALS (csrc/als.hip, THE CONTRACT in include/ncf_abi.h): ``n_iters`` iterations of the user half-sweep followed
    by the item half-sweep, each row the exact minimiser ``(Y^T Y + sum (alpha v) y y^T + reg I)^-1 sum (1 + alpha v) y`` by Cholesky.
    ``fit`` / ``fit_dataset`` / ``fit_csr``; then ``as_mf()`` (the project's MF with the two tables: every ranking and evaluation
    function takes it), ``predict``, ``fold_in_users`` (the exact vectors of new users against the fixed item table) and
    ``recommend_new_users``.  A fit is a fixed function of its inputs, bit for bit.  There is no host path."""

    def __init__(self, n_factors=64, n_iters=15, reg=0.01, alpha=40.0, init_sd=0.01):
        who = "ImplicitALS"
        self.n_factors = _int_in(who, n_factors, "n_factors", 1, native.ALS_MAX_FACTORS)
        self.n_iters = _int_in(who, n_iters, "n_iters", 0, INT_MAX)
        self.reg, self.alpha, self.init_sd = _finite(who, reg, "reg", 0.0), _finite(who, alpha, "alpha", 0.0), _finite(who, init_sd, "init_sd", 0.0)
        if not self.reg > 0:
            raise ValueError(f"{who}: reg = {reg} is not > 0")
        self.user_factors_ = self.item_factors_ = None      # (U, F) / (I, F) fp32
        self.item_gram_ = None                              # (F, F) fp32 Gram matrix of the item table: what fold-in solves against
        self.loss_ = []
        self._mf = None

    # ------------------------------------------------------------------ fit
    def fit_csr(self, rowptr, col, val, num_items, generator: Optional[torch.Generator] = None, track_loss: bool = False,
                block_bytes: int = native.ALS_BLOCK_BYTES):
        """Fits on a user CSR on the GPU: ``rowptr`` (U + 1) int64, ``col`` int32 item positions strictly ascending inside a row,
        ``val`` fp32 >= 0 (SparseRatings' arrays as they are).  The tables start as N(0, init_sd) draws from ``generator`` (one
        normal_ of (U, F), then one of (I, F), on the generator's device), rows without any entry as zeros, which they stay.  With
        ``track_loss``, ``loss_`` holds the float64 objective after every half-sweep (a diagnostic by torch operations; it
        synchronises once at the end).  ``block_bytes`` sizes the scratch buffer of rows longer than a segment and changes no bit."""
        rowptr, col, val, I, dev = self._csr(rowptr, col, val, num_items)
        F, U = self.n_factors, rowptr.numel() - 1
        colptr, row, tval = build_transpose(rowptr, col, val, I)
        tables = []
        for rows, ptr in ((U, rowptr), (I, colptr)):
            gdev = generator.device if generator is not None else dev
            t = torch.empty((rows, F), dtype=torch.float32, device=gdev).normal_(0.0, self.init_sd, generator=generator).to(dev)
            t[ptr[1:] == ptr[:-1]] = 0.0
            tables.append(t)
        X, Y = tables
        users, items = torch.arange(U, device=dev), torch.arange(I, device=dev)
        plan_u, plan_i = native.als_plan(rowptr, users, F, block_bytes), native.als_plan(colptr, items, F, block_bytes)
        entry_user = torch.repeat_interleave(users, rowptr[1:] - rowptr[:-1]) if track_loss else None
        losses = []
        for _ in range(self.n_iters):
            native.als_solve_rows(rowptr, col, val, users, Y, native.als_gram(Y), self.alpha, self.reg, out=X, out_by_row=True, plan=plan_u)
            if track_loss:
                losses.append(self._objective(entry_user, col, val, X, Y))
            native.als_solve_rows(colptr, row, tval, items, X, native.als_gram(X), self.alpha, self.reg, out=Y, out_by_row=True, plan=plan_i)
            if track_loss:
                losses.append(self._objective(entry_user, col, val, X, Y))
        self.user_factors_, self.item_factors_, self.item_gram_ = X, Y, native.als_gram(Y)
        self.num_users_, self.num_items_, self._mf = U, I, None
        self.loss_ = [float(v) for v in torch.stack(losses).cpu()] if losses else []
        self.check()
        return self

    def _objective(self, entry_user, col, val, X, Y, chunk=1 << 20):
        """sum over the entries of c (1 - s)^2 - s^2, + sum_u x_u^T (Y^T Y) x_u, + reg (|X|^2 + |Y|^2) as a float64 device scalar, with
        the alpha and reg the kernels see (their fp32 values)."""
        alpha, reg = float(np.float32(self.alpha)), float(np.float32(self.reg))
        X64, Y64 = X.double(), Y.double()
        acc = ((X64 @ (Y64.t() @ Y64)) * X64).sum() + reg * ((X64 * X64).sum() + (Y64 * Y64).sum())
        for e0 in range(0, col.numel(), chunk):
            e1 = min(col.numel(), e0 + chunk)
            s = (X64[entry_user[e0:e1]] * Y64[col[e0:e1].long()]).sum(1)
            c = 1.0 + alpha * val[e0:e1].double()
            acc = acc + (c * (1.0 - s) ** 2 - s * s).sum()
        return acc

    def fit(self, user_pos, item_pos, rating, num_users, num_items, generator: Optional[torch.Generator] = None, track_loss: bool = False,
            **fit_args):
        """Fits on int64 positions and fp32 values that live on the GPU (KernelMF.fit's arguments): the CSR is built on the device by
        a stable sort on (user, item).  A (user, item) pair given twice raises in check()."""
        _, num_users, num_items, _ = self._samples(user_pos, item_pos, rating, num_users, num_items)
        rowptr, col, val = build_csr(user_pos, item_pos, rating, num_users, num_items)
        return self.fit_csr(rowptr, col, val, num_items, generator=generator, track_loss=track_loss, **fit_args)

    def check(self):
        """Synchronises.  Raises when a half-sweep of this device met what it refuses (native.check_als): ValueError for a row whose
        columns do not strictly ascend (a pair given twice), a value that is negative or not finite or a pivot that is not positive,
        IndexError for an id or a pointer outside its array; each raises once and is then cleared."""
        self._fitted()
        native.check_als(self.user_factors_.device)

    def _fitted(self):
        if self.user_factors_ is None:
            raise RuntimeError("ImplicitALS: not fitted")

    # ------------------------------------------------------------------ scoring
    def as_mf(self):
        """The project's MF module over the two tables (score = x_u . y_i), zero Linear biases, frozen and in eval mode, on the fit's
        device.  top_k_items, rank_of_items, eval_full_ranking and [state_dict, kwargs] checkpoints work on it as on any MF."""
        self._fitted()
        if self._mf is None:
            self._mf = _mf_of_tables(self.user_factors_, self.item_factors_)
        return self._mf

    def predict(self, user_pos, item_pos):
        """(n,) preference scores x_u . y_i for int64 positions on the fit's device: as_mf()'s forward."""
        _positions("ImplicitALS.predict", user_pos, "user_pos")
        _positions("ImplicitALS.predict", item_pos, "item_pos", user_pos.numel())
        with torch.no_grad():
            return self.as_mf()(user_pos.contiguous(), item_pos.contiguous()).view(-1)

    # ------------------------------------------------------------------ fold-in
    def fold_in_users(self, ratings, user_rows, block_bytes: int = native.ALS_BLOCK_BYTES):
        """(B, F) fp32 vectors of the rows ``user_rows`` (int64) of ``ratings`` — a SparseRatings or a (rowptr, col, val) tuple over the
        fitted items, not necessarily the fitted ratings, so new users work: one half-sweep against the fixed item table and its
        cached Gram matrix, the exact minimiser for each row.  A row without entries gives zeros.  Call check() to learn of refused
        input."""
        self._fitted()
        rowptr, col, val = _ratings_csr("ImplicitALS.fold_in_users", ratings)
        _positions("ImplicitALS.fold_in_users", user_rows, "user_rows")
        return native.als_solve_rows(rowptr, col, val, user_rows.contiguous(), self.item_factors_, self.item_gram_, self.alpha, self.reg,
                                     block_bytes=block_bytes)

    def recommend_new_users(self, ratings, user_rows, k, exclude_rated=True, **top_k_args):
        """``top_k_items``' tuple ``(scores (B, k), item_positions (B, k) int64, counts (B,) int32)`` for the rows ``user_rows`` of
        ``ratings`` folded in: the ``k`` best items of an MF over the folded vectors and the fitted item table, the rows' own items left
        out with ``exclude_rated``."""
        from . import recommend
        vectors = self.fold_in_users(ratings, user_rows)
        rowptr, col, _ = _ratings_csr("ImplicitALS.recommend_new_users", ratings)
        exclude = recommend.rated_exclusion(SimpleNamespace(rowptr=rowptr, col=col), user_rows) if exclude_rated else None
        users = torch.arange(user_rows.numel(), device=vectors.device)
        return recommend.top_k_items(_mf_of_tables(vectors, self.item_factors_), users, k, exclude=exclude, **top_k_args)


# ---------------------------------------------------------------------------------------- EASE and SLIM
def _gram_matrix(rowptr, col, val, I, dev, block_bytes):
    """The dense (I, I) fp32 Gram matrix X^T X of a checked user CSR: ncf_ease_gram over ``block_bytes`` of rows at a time, which
    changes no bit."""
    colptr, row, tval = build_transpose(rowptr, col, val, I)
    G = torch.empty((I, I), dtype=torch.float32, device=dev)
    rows = max(1, int(block_bytes) // (4 * I))
    for i0 in range(0, I, rows):
        i1 = min(I, i0 + rows)
        native.ease_gram(rowptr, col, val, colptr, row, tval, (i0, i1), out=G[i0:i1])
    return G


class _ItemItem(_Baseline):
    """What the models with a dense item-item matrix ``weights_`` (I, I) fp32, rows = source items, share: ``fit`` from samples,
    the Gram-side checks, and the serving through ncf_ease_scores / ncf_ease_predict / topk_rows.  ``binary`` models read every
    stored entry as 1.0."""

    def fit(self, user_pos, item_pos, rating, num_users, num_items, **fit_args):
        """Fits on int64 positions and fp32 ratings that live on the GPU (KernelMF.fit's arguments): the CSR is built on the device by
        a stable sort on (user, item).  A (user, item) pair given twice raises in check()."""
        _, num_users, num_items, _ = self._samples(user_pos, item_pos, rating, num_users, num_items)
        rowptr, col, val = build_csr(user_pos, item_pos, rating, num_users, num_items)
        return self.fit_csr(rowptr, col, val, num_items, **fit_args)

    def _fitted(self):
        if self.weights_ is None:
            raise RuntimeError(f"{type(self).__name__}: not fitted")

    def _ratings(self, who, ratings):
        rowptr, col, val = _ratings_csr(who, ratings)
        return rowptr, col, (torch.ones_like(val) if self.binary else val)

    def scores(self, ratings, user_rows, item_range=None, stage_cap: int = 0):
        """(B, i1 - i0) fp32 scores of the rows ``user_rows`` (int64) of ``ratings`` — a SparseRatings or a (rowptr, col, val) tuple
        over the fitted items, not necessarily the fitted ratings, so new users work — against the items ``item_range`` = (i0, i1)
        (default: all).  A ``binary`` model reads every stored entry as 1.0."""
        self._fitted()
        rowptr, col, val = self._ratings(f"{type(self).__name__}.scores", ratings)
        return native.ease_scores(rowptr, col, val, user_rows.contiguous() if torch.is_tensor(user_rows) else user_rows, self.weights_,
                                  item_range, stage_cap)

    def predict(self, ratings, user_rows, item_pos):
        """(n,) fp32 scores of the pairs (row ``user_rows[k]`` of ``ratings``, item ``item_pos[k]``), int64 both: ``scores``' values bit
        for bit."""
        self._fitted()
        rowptr, col, val = self._ratings(f"{type(self).__name__}.predict", ratings)
        return native.ease_predict(rowptr, col, val, user_rows, item_pos, self.weights_)

    def similar_items(self, item_pos, k: int):
        """"More like this": ``(scores (n, k) fp32, item_positions (n, k) int64, counts (n,) int32)`` — the ``k`` largest entries of
        the listed rows of ``weights_``, in ``top_k_items``' form and order (native.topk_rows)."""
        self._fitted()
        _positions(f"{type(self).__name__}.similar_items", item_pos, "item_pos")
        s, idx, cnt = native.topk_rows(self.weights_.index_select(0, item_pos), k)
        return s, idx.to(torch.int64), cnt


class EASE(_ItemItem):
    """The closed-form item-item autoencoder (csrc/ease.hip, THE CONTRACT in include/ncf_abi.h): ``weights_`` = W with
    ``W[i][j] = -P[i][j] / P[j][j]`` off the diagonal and 0 on it, ``P = (X^T X + reg 1)^-1``, and scores ``X W``.  ``binary`` fits on
    1.0 for every stored entry.  ``fit`` / ``fit_dataset`` / ``fit_csr`` (with ``at_regs``: one model per reg from one Gram matrix);
    then ``scores``, ``predict``, ``similar_items``; ``recommend.ease_top_k`` / ``ease_ranks`` rank with it.  A fit is a fixed
    function of its inputs, bit for bit.  There is no host path."""

    def __init__(self, reg=500.0, binary=False):
        who = "EASE"
        self.reg = _finite(who, reg, "reg", 0.0)
        if not self.reg > 0:
            raise ValueError(f"{who}: reg = {reg} is not > 0")
        if not isinstance(binary, (bool, np.bool_)):
            raise ValueError(f"{who}: binary = {binary!r} is not a bool")
        self.binary = bool(binary)
        self.weights_ = None                                # (I, I) fp32
        self.num_items_ = None

    # ------------------------------------------------------------------ fit
    def fit_csr(self, rowptr, col, val, num_items, block_bytes: int = 256 << 20, at_regs: Optional[Sequence[float]] = None):
        """Fits on a user CSR on the GPU: ``rowptr`` (U + 1) int64, ``col`` int32 item positions strictly ascending inside a row,
        ``val`` fp32 (SparseRatings' arrays as they are).  The Gram rows are computed ``block_bytes`` at a time, which changes no
        bit.  With ``at_regs`` the Gram matrix is computed once and a list of fitted models is returned, one per reg, each with the
        bits of its own fit; otherwise this model is fitted and returned.  Synchronises once, in check()."""
        regs = None if at_regs is None else [EASE(reg=r, binary=self.binary).reg for r in at_regs]
        rowptr, col, val, I, dev = self._csr(rowptr, col, val, num_items)
        if I > native.EASE_MAX_ITEMS:
            raise ValueError(f"EASE: {I} items (at most {native.EASE_MAX_ITEMS})")
        if self.binary:
            val = torch.ones_like(val)
        G = _gram_matrix(rowptr, col, val, I, dev, block_bytes)
        if regs is None:
            self._finish(G, I)
            return self
        models = []
        for k, reg in enumerate(regs):
            m = EASE(reg=reg, binary=self.binary)
            m._finish(G.clone() if k + 1 < len(regs) else G, I)
            models.append(m)
        return models

    def _finish(self, G, I):
        """G -> weights_, in place, and the check."""
        self.weights_, self.num_items_ = native.ease_weights(native.ease_invert(G, self.reg)), I
        self.check()

    def check(self):
        """Synchronises.  Raises ValueError when a fit walked a row whose columns do not strictly ascend or met a pivot that is not
        positive and finite (the weights are then zeros), and IndexError when a kernel of this device met an id outside its range;
        each raises once and is then cleared."""
        self._fitted()
        dev = self.weights_.device
        native.check_ease(dev)
        native.check_oob(dev)


# ---------------------------------------------------------------------------------------- SLIM
class SLIM(_ItemItem):
    """Sparse linear item-item weights (csrc/slim.hip, THE CONTRACT in include/ncf_abi.h): column j of ``weights_`` minimises
    ``1/2 |x_j - X w|^2 + 1/2 l2_reg |w|^2 + l1_reg |w|_1`` with ``w[j] = 0`` — and ``w >= 0`` with ``positive`` — by cyclic
    coordinate descent on the Gram matrix, at most ``max_sweeps`` sweeps, until a sweep moves no weight by more than ``tol``.
    ``binary`` fits on 1.0 for every stored entry.  ``fit`` / ``fit_dataset`` / ``fit_csr`` (with ``at_regs``: one model per
    (l1, l2) from one Gram matrix); then ``scores``, ``predict``, ``similar_items``; ``recommend.slim_top_k`` / ``slim_ranks`` rank
    with it.  After a fit: ``sweeps_`` / ``steps_`` (I,) int32 and ``last_delta_`` (I,) fp32 per item's column, and, from
    ``check()``, ``density_`` (the share of ``weights_`` that is not zero) and ``n_unconverged_`` (columns whose last sweep still
    moved a weight by more than ``tol``; not an error).  A fit is a fixed function of its inputs, bit for bit the serial loop.
    There is no host path."""

    def __init__(self, l1_reg, l2_reg, positive=True, max_sweeps=100, tol=1e-4, binary=False):
        who = "SLIM"
        self.l1_reg, self.l2_reg = _finite(who, l1_reg, "l1_reg", 0.0), _finite(who, l2_reg, "l2_reg", 0.0)
        self.tol = _finite(who, tol, "tol", 0.0)
        self.max_sweeps = _int_in(who, max_sweeps, "max_sweeps", 1, INT_MAX)
        for v, what in ((positive, "positive"), (binary, "binary")):
            if not isinstance(v, (bool, np.bool_)):
                raise ValueError(f"{who}: {what} = {v!r} is not a bool")
        self.positive, self.binary = bool(positive), bool(binary)
        self.weights_ = None                                # (I, I) fp32, rows = source items
        self.num_items_ = None
        self.sweeps_ = self.steps_ = self.last_delta_ = None
        self.density_ = self.n_unconverged_ = None

    @classmethod
    def elastic_net(cls, alpha, l1_ratio, num_users, **kw):
        """The model of scikit-learn's ``ElasticNet(alpha, l1_ratio)`` fitted per item on ``num_users`` rows, whose objective is this
        one divided by the number of rows: ``l1_reg = alpha * l1_ratio * num_users``, ``l2_reg = alpha * (1 - l1_ratio) * num_users``."""
        who = "SLIM.elastic_net"
        alpha, l1_ratio = _finite(who, alpha, "alpha", 0.0), _finite(who, l1_ratio, "l1_ratio", 0.0)
        if l1_ratio > 1:
            raise ValueError(f"{who}: l1_ratio = {l1_ratio} is not in 0 .. 1")
        U = _int_in(who, num_users, "num_users", 1, INT_MAX)
        return cls(alpha * l1_ratio * U, alpha * (1.0 - l1_ratio) * U, **kw)

    def _like(self, l1_reg, l2_reg):
        return SLIM(l1_reg, l2_reg, positive=self.positive, max_sweeps=self.max_sweeps, tol=self.tol, binary=self.binary)

    # ------------------------------------------------------------------ fit
    def fit_csr(self, rowptr, col, val, num_items, block_bytes: int = 256 << 20, at_regs: Optional[Sequence] = None,
                warm_path: bool = False):
        """Fits on a user CSR on the GPU: ``rowptr`` (U + 1) int64, ``col`` int32 item positions strictly ascending inside a row,
        ``val`` fp32 (SparseRatings' arrays as they are).  The Gram rows are computed ``block_bytes`` at a time, which changes no
        bit; the columns are handed to the solver heaviest first (descending ``G[j][j]``, ties by position), which changes none
        either.  With ``at_regs`` = [(l1, l2), ...] the Gram matrix is computed once and a list of fitted models is returned, one per
        point, each a cold fit with the bits of its own fit.  With ``warm_path`` every point after the first starts from the
        weights of the point before it: fewer sweeps along a path of falling penalties, but the bits of a point then depend on the
        path that led to it.  Synchronises in check(), once per fitted model."""
        if not isinstance(warm_path, (bool, np.bool_)):
            raise ValueError(f"SLIM: warm_path = {warm_path!r} is not a bool")
        if at_regs is not None and not all(isinstance(r, (tuple, list)) and len(r) == 2 for r in at_regs):
            raise ValueError("SLIM: at_regs must hold (l1_reg, l2_reg) pairs")
        models = None if at_regs is None else [self._like(*r) for r in at_regs]
        if isinstance(num_items, bool) or not isinstance(num_items, numbers.Integral):
            raise ValueError(f"SLIM: num_items = {num_items!r} is not an integer")
        if num_items > native.SLIM_MAX_ITEMS:                # before anything is converted or allocated
            raise ValueError(f"SLIM: {int(num_items)} items (at most {native.SLIM_MAX_ITEMS})")
        rowptr, col, val, I, dev = self._csr(rowptr, col, val, num_items)
        if self.binary:
            val = torch.ones_like(val)
        G = _gram_matrix(rowptr, col, val, I, dev, block_bytes)
        order = torch.argsort(G.diagonal(), descending=True, stable=True).to(torch.int32)
        Wt = None
        for m in [self] if models is None else models:
            warm = bool(warm_path) and Wt is not None
            Wt = m._solve(G, order, Wt if warm else None)
        return self if models is None else models

    def _solve(self, G, order, Wt):
        """One solve of every column, warm from ``Wt`` (then updated in place) when given; sets the fitted attributes and checks."""
        warm = Wt is not None
        if not warm:                                         # `order` lists every column once, and a cold solve writes the whole of each listed row
            Wt = torch.empty_like(G)
        Wt, sweeps, steps, last = native.slim_solve(G, self.l1_reg, self.l2_reg, order, self.positive, warm, self.max_sweeps, self.tol,
                                                    out=Wt)
        by_item = order.to(torch.int64)
        self.sweeps_, self.steps_, self.last_delta_ = (torch.empty_like(t).index_copy_(0, by_item, t) for t in (sweeps, steps, last))
        self.weights_, self.num_items_ = Wt.t().contiguous(), G.shape[0]
        self.check()
        return Wt

    def check(self):
        """Synchronises.  Raises ValueError when a fit walked a row whose columns do not strictly ascend, and IndexError when a kernel
        of this device met an id outside its range; each raises once and is then cleared.  A column that met ``max_sweeps`` raises
        nothing: it is counted in ``n_unconverged_``, which this sets together with ``density_``."""
        self._fitted()
        dev = self.weights_.device
        native.check_ease(dev)
        native.check_oob(dev)
        self.density_ = float(torch.count_nonzero(self.weights_).item()) / float(self.weights_.numel())
        self.n_unconverged_ = int((self.last_delta_ > self.tol).sum().item())
