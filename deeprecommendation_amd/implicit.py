"""Implicit-feedback training and sampled evaluation, the protocol of the NCF paper (He et al. 2017): every interaction is a
positive, each positive meets ``negatives`` items the user has NOT interacted with, drawn uniformly and redrawn every epoch, the
loss is the log loss (or BPR over the same pairs), and a model is reported by HR@10 / NDCG@10 of one held-out item per user among
99 sampled unseen items.  The reference trains on explicit ratings only; ``ImplicitALS`` (baselines.py) is the classical model this
sets the neural ones against.

``leave_one_out``       the split: one held-out item per user, on the host.
``ImplicitFeedback``    the distinct positives and their sorted CSR on the device; ``negatives`` is one ``native.sample_unseen`` call
                        (csrc/unseen.hip, THE CONTRACT in include/ncf_abi.h): no rejection rounds, no host read.
``fit_implicit``        the epoch loop in ``train_model``'s resident style for BasicNCF / MF / GraphNCF on index ids; loss="softmax"
                        (the dot-product models) scores each positive against the whole catalogue and draws no negatives.
``sampled_candidates``  each user's fixed candidate list; ``eval_sampled`` ranks the held-out item in it (``rank_sampled``: the ranks).

Users and items are POSITIONS throughout: 0 .. n_users - 1 and 0 .. n_items - 1, the rows and columns of the seen CSR.  Everything past
the split runs on the GPU; there is no host path."""
from __future__ import annotations

import numbers
from typing import Callable, Optional, Sequence

import numpy as np
import torch

from . import native
from .baselines import build_csr

_M32 = 0xFFFFFFFF
LOSSES = ("bce", "bpr", "softmax")


def _lowbias32(x: np.ndarray) -> np.ndarray:
    """The header's mix (include/ncf_abi.h, under ncf_sample_negatives) on uint32 values carried in uint64."""
    x = x & np.uint64(_M32)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & np.uint64(_M32)
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & np.uint64(_M32)
    return x ^ (x >> np.uint64(16))


def slot_hash(seed: int, slots) -> np.ndarray:
    """The two-round hash of (seed, slot) every sampler of the library starts from, as uint64 values below 2^32."""
    s = np.asarray(slots, dtype=np.uint64)
    x = _lowbias32(((s & np.uint64(_M32)) * np.uint64(0x9E3779B1)) ^ np.uint64(int(seed) & _M32))
    return _lowbias32(x ^ (((s >> np.uint64(32)) * np.uint64(0x85EBCA77)) & np.uint64(_M32)) ^ np.uint64(0x68E31DA4))


def epoch_seed(seed: int, epoch: int) -> int:
    """The sampler's seed of ``epoch`` (from 0) under ``fit_implicit(seed=...)``: the hash of (seed, epoch), so that two epochs share
    no stream of draws."""
    return int(slot_hash(seed, [epoch])[0])


def _host_positions(who, t, what):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    if a.ndim != 1 or a.dtype.kind not in "iu":
        raise ValueError(f"{who}: {what} must be a 1-D array of integer positions")
    return a.astype(np.int64)


def leave_one_out(user_pos, item_pos, timestamps=None, seed: int = 0):
    """The leave-one-out split of implicit feedback, on the host: ``(train_users, train_items, held_users, held_items)``, int64
    numpy arrays, the training pairs in (user, item) order and the held-out pairs in user order.

    A (user, item) pair given twice counts once (with ``timestamps``: at its latest one).  With ``timestamps`` a user's held-out item
    is the latest interaction, a tie going to the larger item position; without, it is entry ``(h * n) >> 32`` of the user's n
    distinct items in ascending order, h the library's hash of (seed, user) (``slot_hash``): the same split for the same seed.  A
    user with fewer than two distinct items keeps them all in training and has no held-out item."""
    who = "leave_one_out"
    u, i = _host_positions(who, user_pos, "user_pos"), _host_positions(who, item_pos, "item_pos")
    if len(u) != len(i):
        raise ValueError(f"{who}: user_pos has {len(u)} entries, item_pos {len(i)}")
    if len(u) and (u.min() < 0 or i.min() < 0):
        raise ValueError(f"{who}: a position is negative")
    if timestamps is not None:
        t = timestamps.detach().cpu().numpy() if torch.is_tensor(timestamps) else np.asarray(timestamps)
        if t.shape != u.shape:
            raise ValueError(f"{who}: timestamps has shape {t.shape}, expected {u.shape}")
        order = np.lexsort((t, i, u))                       # by user, then item, then time: a pair's last entry is its latest
        u, i, t = u[order], i[order], t[order]
        last = np.ones(len(u), dtype=bool)
        last[:-1] = (u[1:] != u[:-1]) | (i[1:] != i[:-1])
        u, i, t = u[last], i[last], t[last]
    else:
        order = np.lexsort((i, u))
        u, i = u[order], i[order]
        first = np.ones(len(u), dtype=bool)
        first[1:] = (u[1:] != u[:-1]) | (i[1:] != i[:-1])
        u, i = u[first], i[first]
    users, start, count = np.unique(u, return_index=True, return_counts=True)
    if timestamps is not None:
        by_time = np.lexsort((i, t, u))                     # within a user: ascending time, ties by ascending item; the last wins
        held = by_time[start + count - 1]
    else:
        held = start + ((slot_hash(seed, users) * count.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
    held = held[count >= 2]
    keep = np.ones(len(u), dtype=bool)
    keep[held] = False
    return u[keep], i[keep], u[held], i[held]


class ImplicitFeedback:
    """The distinct positives of an implicit-feedback data set on ``device``: ``users`` / ``items`` (n,) int64 in (user, item)
    order, and their CSR over users ``rowptr`` (n_users + 1) int64 / ``col`` int32, ascending inside a row (baselines.build_csr).
    Positions outside ``[0, n_users)`` / ``[0, n_items)`` are refused here, by one host check."""

    def __init__(self, user_pos, item_pos, n_users: int, n_items: int, device="cuda"):
        who = "ImplicitFeedback"
        self.n_users = native._int_in(who, n_users, "n_users", 1, 2 ** 31 - 1)
        self.n_items = native._int_in(who, n_items, "n_items", 1, 2 ** 31 - 1)
        u, i = _host_positions(who, user_pos, "user_pos"), _host_positions(who, item_pos, "item_pos")
        if len(u) != len(i) or len(u) == 0:
            raise ValueError(f"{who}: user_pos has {len(u)} entries, item_pos {len(i)} (one length, not empty)")
        if u.min() < 0 or u.max() >= self.n_users or i.min() < 0 or i.max() >= self.n_items:
            raise ValueError(f"{who}: a position lies outside the {self.n_users} users or the {self.n_items} items")
        key = np.unique(u * self.n_items + i)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"{who} lives on the GPU (got {self.device}); there is no CPU path")
        self.users = torch.from_numpy(key // self.n_items).to(self.device)
        self.items = torch.from_numpy(key % self.n_items).to(self.device)
        self.n = int(key.size)
        self.rowptr, self.col, _ = build_csr(self.users, self.items, self.items, self.n_users, self.n_items)

    def __len__(self):
        return self.n

    @property
    def seen(self):
        """The seen CSR ``(rowptr, col)`` as the kernels take it."""
        return self.rowptr, self.col

    def negatives(self, pick_users: torch.Tensor, k: int, seed: int, slot0: int = 0) -> torch.Tensor:
        """``(n, k)`` int64: k distinct unseen items for each listed user, the draw of ``native.sample_unseen`` for the slots
        slot0 .. slot0 + n - 1.  No synchronisation; ``check`` reports a refused row."""
        return native.sample_unseen(self.seen, self.n_items, pick_users, k, seed, slot0)

    def exclusion(self, users: torch.Tensor, extra_items: Optional[torch.Tensor] = None):
        """The seen CSR ``(rowptr (B + 1) int64, col int32)`` of the listed users, row b for users[b], each row ascending; with
        ``extra_items`` (B,) int64, row b also holds extra_items[b] in its sorted place (once, if the user has seen it) — the held-out
        item, which a sampled candidate must not be.  Torch ops on the device; sizes its result on the host."""
        who = "ImplicitFeedback.exclusion"
        if not torch.is_tensor(users) or users.dtype != torch.int64 or users.dim() != 1:
            raise ValueError(f"{who}: users must be a 1-D int64 tensor")
        B = users.numel()
        if extra_items is not None and not (torch.is_tensor(extra_items) and extra_items.dtype == torch.int64 and tuple(extra_items.shape) == (B,)):
            raise ValueError(f"{who}: extra_items must be a ({B},) int64 tensor")
        users = users.to(self.device)
        lo = self.rowptr[users]
        cnt = self.rowptr[users + 1] - lo
        row = torch.repeat_interleave(torch.arange(B, device=self.device), cnt)
        start = torch.cumsum(cnt, 0) - cnt
        entry = lo[row] + torch.arange(row.numel(), device=self.device) - start[row]
        key = row * self.n_items + self.col[entry].to(torch.int64)
        if extra_items is not None:
            key = torch.unique(torch.cat([key, torch.arange(B, device=self.device) * self.n_items + extra_items.to(self.device)]))
        rowptr = torch.zeros(B + 1, dtype=torch.int64, device=self.device)
        rowptr[1:] = torch.cumsum(torch.bincount(torch.div(key, self.n_items, rounding_mode="floor"), minlength=B), 0)
        return rowptr, (key % self.n_items).to(torch.int32)

    def check(self):
        """Synchronises.  Raises what a draw on this device refused (native.check_unseen: IndexError for a pick outside the users,
        ValueError for a user with fewer unseen items than the draws asked for) and IndexError for an id outside an embedding table;
        each raises once and is then cleared."""
        native.check_unseen(self.device)
        native.check_oob(self.device)


def _scorer(who, model, graph):
    """``score(users, items)`` of a supported model over user and item POSITIONS, or TypeError naming them.  A GraphNCF scores
    graph nodes, where user u is node graph.num_items + u (IndexGraphProvider.get_user_nodeID): the offset is added here."""
    from .neural_collaborative_filtering.models.basic_ncf import BasicNCF
    from .neural_collaborative_filtering.models.gnn_ncf import GraphNCF
    from .neural_collaborative_filtering.models.mf import MF
    from .neural_collaborative_filtering.models.neumf import NeuMF
    if isinstance(model, GraphNCF):
        if graph is None:
            raise ValueError(f"{who}: a GraphNCF needs graph=")
        if not hasattr(graph, "num_items"):
            raise ValueError(f"{who}: graph= must be the provider's GraphData")
        return lambda u, i: model(graph.to(u.device), u + graph.num_items, i)
    if isinstance(model, (BasicNCF, MF, NeuMF)):
        if graph is not None:
            raise ValueError(f"{who}: graph= goes with a GraphNCF, not a {type(model).__name__}")
        return model
    raise TypeError(f"{who}: takes a BasicNCF, a NeuMF or an MF in index form (forward(users, items)) or a GraphNCF with graph= "
                    f"(forward(graph, users, items)), not a {type(model).__name__}")


def _softmax_scorer(who, model, graph):
    """``loss(users, items)`` (per-row full-catalogue softmax loss over POSITIONS) of a dot-product model, or TypeError naming them."""
    from .neural_collaborative_filtering.models.gnn_ncf import GraphNCF
    from .neural_collaborative_filtering.models.mf import MF
    if isinstance(model, GraphNCF) and model.MLP is None:
        return lambda u, i, scale: model.softmax_loss(graph.to(u.device), u + graph.num_items, i, scale)
    if isinstance(model, MF):
        return model.softmax_loss
    raise TypeError(f'{who}: loss = "softmax" takes a dot-product model, an MF or a GraphNCF(use_dot_product=True), not a '
                    f"{type(model).__name__}" + (" with an MLP readout" if isinstance(model, GraphNCF) else ""))


def fit_implicit(model, data: ImplicitFeedback, *, negatives: int = 4, loss: str = "bce", epochs: int, batch_size: int, lr: float,
                 weight_decay: float = 0.0, optimizer=None, graph=None, seed: Optional[int] = None, shuffle: bool = True,
                 on_epoch: Optional[Callable] = None, scale: float = 1.0) -> dict:
    """Trains ``model`` on the positives of ``data`` against unseen negatives drawn on the device, in ``train_model``'s resident style:
    per epoch one permutation drawn on the device, a batch is a gather of positives plus ONE ``native.sample_unseen`` call (slots
    numbered across the epoch, so the draw does not depend on the batch size), the running loss stays on the device (one host read
    per epoch) and the sampler's flag is checked after the epoch.

    loss="bce": one forward over the batch's B positives followed by its B * negatives negatives (row b's in order), labels 1 and 0,
    ``BCEWithLogitsLoss(reduction="sum")``; ``train_loss`` divides the epoch's sum by its n * (1 + negatives) scored pairs.
    loss="bpr": the same forward; each positive's score is paired with each of its negatives' under
    ``RankingDataset.calculate_loss`` (sum of -log sigmoid(pos - neg)); ``train_loss`` divides by the n * negatives pairs.
    loss="softmax" (MF, GraphNCF(use_dot_product=True); another model raises TypeError): softmax cross-entropy of each positive
    over the WHOLE catalogue, ``model.softmax_loss(u, i, scale)`` summed over the batch (autograd.DotSoftmaxLossFn: the B x n_items
    logits are never built); no negatives are drawn and ``negatives`` is ignored; ``scale`` (finite, > 0) multiplies the logits;
    ``train_loss`` divides the epoch's sum by its n positives.  ``batch_size`` is at most native.DOT_SOFTMAX_MAX_ROWS (65 536, the
    rows one ncf_dot_lse call takes); a larger one raises ValueError.  The loss kernels use no float atomics and the user rows'
    gradients are summed in a fixed order when the embedding width is a multiple of 4, so an MF of such a width fitted twice from
    the same state of torch's generators gives the same bits (tests/test_gpu_dot_softmax.py); another width keeps the atomic row
    scatter, and a GraphNCF's step is as repeatable as its propagation backward, which this loss does not change.
    The sampler's seed is drawn per epoch from torch's host generator, or is ``epoch_seed(seed, epoch)`` when ``seed`` is given.
    The optimiser defaults to ``FusedAdam(lr, weight_decay)``.  ``on_epoch(epoch, model)`` runs after every epoch (evaluate there);
    training stops when it returns False.  Returns ``{"train_loss": [...]}``."""
    who = "fit_implicit"
    score = _scorer(who, model, graph)
    if loss not in LOSSES:
        raise ValueError(f"{who}: loss = {loss!r} (one of {', '.join(LOSSES)})")
    softmax = _softmax_scorer(who, model, graph) if loss == "softmax" else None
    scale = native._finite(who, scale, "scale")
    if not scale > 0:
        raise ValueError(f"{who}: scale = {scale!r} is not > 0")
    K = 0 if softmax else native._int_in(who, negatives, "negatives", 1, native.UNSEEN_MAX_K)
    epochs = native._int_in(who, epochs, "epochs", 0, 2 ** 31 - 1)
    batch_size = native._int_in(who, batch_size, "batch_size", 1, native.DOT_SOFTMAX_MAX_ROWS if softmax else 2 ** 31 - 1)
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, numbers.Integral)):
        raise ValueError(f"{who}: seed = {seed!r} is not an integer")
    if not isinstance(data, ImplicitFeedback):
        raise TypeError(f"{who}: data must be an ImplicitFeedback, not a {type(data).__name__}")
    from .neural_collaborative_filtering.datasets.base import BPR_loss
    dev, n = data.device, data.n
    model.to(dev)
    if optimizer is None:
        from .optim import FusedAdam
        optimizer = FusedAdam(model.parameters(), lr=lr, weight_decay=weight_decay)
    bce = torch.nn.BCEWithLogitsLoss(reduction="sum")
    scored = n if softmax else n * (1 + K) if loss == "bce" else n * K
    history = {"train_loss": []}
    for epoch in range(epochs):
        model.train()
        order = torch.randperm(n, device=dev) if shuffle else torch.arange(n, device=dev)
        draw_seed = epoch_seed(seed, epoch) if seed is not None else native.host_seed()   # host generator
        running = torch.zeros((), dtype=torch.float64, device=dev)
        for s in range(0, n, batch_size):
            pick = order[s:s + batch_size]
            u, i = data.users[pick], data.items[pick]
            if softmax:
                optimizer.zero_grad()
                batch_loss = softmax(u, i, scale).sum()
                batch_loss.backward()
                optimizer.step()
                running += batch_loss.detach().double()
                continue
            neg = data.negatives(u, K, draw_seed, s)
            B = u.numel()
            optimizer.zero_grad()
            out = score(torch.cat([u, u.repeat_interleave(K)]), torch.cat([i, neg.reshape(-1)])).view(-1)
            if loss == "bce":
                labels = torch.zeros(B * (1 + K), dtype=out.dtype, device=dev)
                labels[:B] = 1.0
                batch_loss = bce(out, labels)
            else:
                batch_loss = BPR_loss(out[:B].repeat_interleave(K), out[B:])
            batch_loss.backward()
            optimizer.step()
            running += batch_loss.detach().double()
        history["train_loss"].append(float(running.item()) / max(1, scored))     # the epoch's only host synchronisation
        data.check()                                                              # the flags, already on the host's side
        if on_epoch is not None and on_epoch(epoch, model) is False:
            break
    return history


def sampled_candidates(data: ImplicitFeedback, users: torch.Tensor, held_out: torch.Tensor, n_candidates: int = 99, seed: int = 0) -> torch.Tensor:
    """``(U, n_candidates)`` int64: for each listed user that many distinct items the user has neither seen nor held out, by one
    ``native.sample_unseen`` call over ``data.exclusion(users, held_out)`` with slot b for users[b].  A fixed function of its arguments:
    draw once, and every epoch and every model is ranked against the same lists.  Synchronises (``data.check()``): a user without
    that many such items raises ValueError."""
    who = "sampled_candidates"
    if not isinstance(data, ImplicitFeedback):
        raise TypeError(f"{who}: data must be an ImplicitFeedback, not a {type(data).__name__}")
    n_candidates = native._int_in(who, n_candidates, "n_candidates", 1, native.UNSEEN_MAX_K)
    excl = data.exclusion(users, held_out)
    out = native.sample_unseen(excl, data.n_items, torch.arange(users.numel(), device=data.device), n_candidates, seed, 0)
    data.check()
    return out


def eval_sampled(model, users: torch.Tensor, held_out: torch.Tensor, candidates: torch.Tensor, cutoffs: Sequence[int] = (10,),
                 graph=None, block_pairs: int = 1 << 20) -> dict:
    """Leave-one-out evaluation with sampled candidates: scores, in eval mode and in blocks of at most ``block_pairs`` pairs, each
    user's ``candidates`` (U, C) int64 and ``held_out`` (U,) int64 item, ranks the held-out item among the C + 1 with
    ``native.rank_rows`` and returns ``ranking_metrics``' dict (``hr@K``, ``recall@K``, ``ndcg@K`` for every K of ``cutoffs``,
    ``mrr``, ``auc``, ``users``; with one target per user recall@K equals hr@K).

    The held-out item is scored in the LAST column.  ``rank_rows`` orders equal scores by column, so a candidate that ties with the
    held-out item comes before it: a tie counts against the model, and a scorer that returns one constant gets rank C and
    HR@K = 0 (for K <= C), not the HR@K = 1 the first column would hand it."""
    from .ranking_eval import ranking_metrics
    cutoffs = [int(K) for K in cutoffs]
    if not cutoffs or min(cutoffs) < 1:
        raise ValueError("eval_sampled: cutoffs must be positive")
    rank, ranked = rank_sampled(model, users, held_out, candidates, graph=graph, block_pairs=block_pairs, who="eval_sampled")
    rowptr = torch.arange(users.numel() + 1, dtype=torch.int64, device=rank.device)
    return ranking_metrics(rank, rowptr, ranked, cutoffs)


def rank_sampled(model, users: torch.Tensor, held_out: torch.Tensor, candidates: torch.Tensor, graph=None, block_pairs: int = 1 << 20,
                 who: str = "rank_sampled"):
    """The ranks ``eval_sampled`` averages: ``(rank (U,) int32, ranked (U,) int32)`` on the device — rank[b] is the number of
    candidates of user b that score higher than the held-out item or equal to it, ranked[b] = C + 1.  No synchronisation."""
    for t, what, nd in ((users, "users", 1), (held_out, "held_out", 1), (candidates, "candidates", 2)):
        if not torch.is_tensor(t) or t.dtype != torch.int64 or t.dim() != nd:
            raise ValueError(f"{who}: {what} must be a {nd}-D int64 tensor")
    U = users.numel()
    if held_out.numel() != U or candidates.shape[0] != U or candidates.shape[1] < 1:
        raise ValueError(f"{who}: {U} users, held_out of {held_out.numel()} entries, candidates of shape {tuple(candidates.shape)}: "
                         f"expected ({U},) and ({U}, C >= 1)")
    block_pairs = native._int_in(who, block_pairs, "block_pairs", 1, 2 ** 62)
    score = _scorer(who, model, graph)
    native._dev_all((users, "users"), (held_out, "held_out"), (candidates, "candidates"))
    dev, C1 = users.device, candidates.shape[1] + 1
    items = torch.cat([candidates, held_out[:, None]], 1)
    rows = max(1, block_pairs // C1)
    was_training = model.training
    model.eval()
    ranks, ranked = [], []
    try:
        for b0 in range(0, U, rows):
            b1 = min(U, b0 + rows)
            with torch.no_grad():
                s = score(users[b0:b1].repeat_interleave(C1), items[b0:b1].reshape(-1)).view(b1 - b0, C1).float().contiguous()
            trow = torch.arange(b1 - b0 + 1, dtype=torch.int64, device=dev)
            tcol = torch.full((b1 - b0,), C1 - 1, dtype=torch.int32, device=dev)
            r, k = native.rank_rows(s, (trow, tcol))
            ranks.append(r), ranked.append(k)
    finally:
        model.train(was_training)
    empty = torch.empty(0, dtype=torch.int32, device=dev)
    return (torch.cat(ranks) if ranks else empty), (torch.cat(ranked) if ranked else empty)
