"""Full-catalogue ranking evaluation on the device: the protocol BPR-trained MF / NCF / LightGCN-style models are reported with.
Each user's held-out items are ranked against the WHOLE catalogue with the training items excluded, exactly (no cap on the rank),
and HR@K / Recall@K / NDCG@K / MRR / AUC are computed from those ranks.

``rank_of_items``      the exact rank of every held-out item of every listed user (BasicNCF / MF / GraphNCF; AttentionNCF with
                       ``profiles=``, always score-then-rank), through the fused rank
                       kernels (``native.dot_rank`` for a dot-product readout, ``native.mlp_rank`` for an MLP readout: no score
                       matrix) or block by block through the model's scoring path and ``native.rank_rows``.  Stays on the device.
``ranking_metrics``    HR@K, Recall@K, NDCG@K, MRR and AUC from those ranks, in float64 on the ranks' device; one host read.
``eval_full_ranking``  the two composed.
``held_out_items``     the users and the de-duplicated target CSR of a test DataFrame.
``intra_list_diversity`` / ``catalogue_coverage``
                       beyond accuracy: how unlike each other the items of a recommendation list are, and how much of the catalogue
                       the lists of all users reach — what ``diversify_top_k`` trades relevance for.  Torch ops, on the lists' device.

The rank of a target is the number of non-excluded columns that come before it in ``top_k_items``' order (descending score, equal
scores to the lower column, NaN last): the slot it would hold in an unbounded ``top_k_items`` result.  ``eval_ranking`` in
neural_collaborative_filtering/eval.py is a different metric (the reference's NDCG over the items a user rated in the test file)
and is unchanged.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import native
from .recommend import BLOCK_BYTES, _csr, _csr_take, _dot_readout, _fused_tables, _mlp_operands, _rank_blocks, _resolve_ranked, _score_blocks


def _take_rows(rowptr, col, rows):
    """The CSR of a row subset: (rowptr', col', entry) with entry = the place of each kept entry in ``col``.  Sizes its result on
    the host (one read)."""
    lo = rowptr[rows]
    new, entry = _csr_take(lo, rowptr[rows + 1] - lo)
    return new, col[entry], entry


def _fused_ranks(model, r, users, seen, targets, max_targets):
    """The fused route over the model's tables for ``users`` (all of the ranked list's, or a row subset with its own ``seen``), or
    None where a fused kernel's limits do not hold (the caller then scores and ranks, which gives the same integers)."""
    if getattr(model, "scoring_dtype", torch.float32) != torch.float32:
        return None
    with torch.no_grad():
        if _dot_readout(model):
            user_tab, item_tab, ids = _fused_tables(model, r, model._refresh())
            if user_tab.shape[1] > native.DOT_RANK_MAX_D:
                return None
            return native.dot_rank(user_tab, users, item_tab, ids, targets, max_targets, seen)
        ops = _mlp_operands(model, r, users)
        if ops is None:
            return None
        tabA, idxA, tabB, idxB, packed, user_first, gmf = ops
        if not native.mlp_rank_supported(packed, tabA.shape[1], tabB.shape[1], max_targets):
            return None
        if gmf is not None:             # a NeuMF: the same waves with the GMF term
            return native.neumf_rank(tabA, idxA, tabB, idxB, gmf[0], gmf[1], packed, gmf[2], targets, max_targets, seen)
        return native.mlp_rank(tabA, idxA, tabB, idxB, packed, targets, max_targets, seen, user_first=user_first)


def _scored_ranks(model, r, users, seen, targets, block_bytes):
    """Score blocks of users through the model and rank each block's targets in its score rows (native.rank_rows)."""
    return _rank_blocks(_score_blocks(model, r, users, block_bytes), users.numel(), targets, seen)


def rank_of_items(model, user_ids: torch.Tensor, targets: Tuple[torch.Tensor, torch.Tensor], item_ids: Optional[torch.Tensor] = None,
                  exclude: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, *, graph=None, fused: Optional[bool] = None,
                  max_targets: Optional[int] = None, block_bytes: int = BLOCK_BYTES, profiles=None):
    """The exact rank of each user's held-out items against the whole ranked list, for a BasicNCF / MF / NeuMF / GraphNCF model.

    user_ids, item_ids, exclude, graph: as in ``top_k_items`` (int64 positions on the GPU; columns of the ranked list; a GraphNCF
    needs ``graph=``).  targets: the held-out items as a per-user CSR ``(rowptr (B + 1) int64, col int32)`` of columns of the
    ranked list (``held_out_items`` builds it from a test file).
    Returns ``(rank (n_targets,) int32, ranked (B,) int32)`` on the device.  rank[e] is the number of non-excluded columns that come
    before target e in ``top_k_items``' order — the slot it would hold in an unbounded ``top_k_items`` result for its user; a user's
    other targets compete like any column; duplicate targets get the same rank; a target that is excluded or not a column of the
    list gets -1.  ranked[b] is the number of non-excluded columns of user b.
    fused: ``None`` ranks a dot-product readout (MF, GraphNCF-dot) with ``native.dot_rank`` and an MLP readout (BasicNCF,
    GraphNCF-MLP) with ``native.mlp_rank`` (a NeuMF with ``native.neumf_rank``), none of which writes a score matrix; what a fused
    kernel does not take (bf16 scoring, a folded first layer, an MLP shape without a fused instance, width > 256) and ``fused=False`` score the users block by
    block through the model (score blocks under ``block_bytes``) and rank with ``native.rank_rows``.  All routes give the same
    integers.
    profiles: ``(item_features, ratings)`` for an AttentionNCF, as in ``top_k_items``: ``fused`` is then the route of
    ``AttentionNCF.catalogue_scores`` (``table=``), its score blocks are ranked with ``native.rank_rows`` (there is no fused rank
    kernel for this model), and ``max_targets`` is not needed: nothing is read back.
    max_targets: the largest number of targets of one user.  ``None`` reads it from ``targets`` — the one host read of this
    function; a caller in a loop passes it in, and then nothing synchronises with the host (a user with more targets than stated
    sets the sticky flag ``native.check_rank_overflow`` reads and has only its first ``max_targets`` ranked).  Users with more than
    ``native.RANK_MAX_TARGETS`` targets are split off and ranked through ``native.rank_rows``; building that row subset reads its
    size on the host."""
    r = _resolve_ranked(model, user_ids, item_ids, exclude, graph, profiles, fused)
    users, seen, B, dev = r.users, r.seen, r.B, r.users.device
    targets = _csr(targets, B, "targets")
    trow, tcol = targets
    if B == 0:
        return torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
    if r.profiles is not None:
        return _scored_ranks(model, r, users, seen, targets, block_bytes)
    if max_targets is None:
        max_targets = int((trow[1:] - trow[:-1]).max().item())          # the one host read
    max_targets = int(max_targets)
    cap = native.RANK_MAX_TARGETS
    out = None
    if fused is None or fused:
        if max_targets <= cap:
            out = _fused_ranks(model, r, users, seen, targets, max(1, max_targets))
        else:
            # the users above the fused cap take the unfused route as a row subset, the others the fused one
            cnt = trow[1:] - trow[:-1]
            small, big = torch.nonzero(cnt <= cap).flatten(), torch.nonzero(cnt > cap).flatten()
            s_row, s_col, s_entry = _take_rows(trow, tcol, small)
            s_seen = None if seen is None else _take_rows(seen[0], seen[1], small)[:2]
            part = _fused_ranks(model, r, users[small].contiguous(), s_seen, (s_row, s_col), cap) \
                if small.numel() else (s_col, small.to(torch.int32))
            if part is not None:
                b_row, b_col, b_entry = _take_rows(trow, tcol, big)
                b_seen = None if seen is None else _take_rows(seen[0], seen[1], big)[:2]
                b_rank, b_ranked = _scored_ranks(model, r, users[big].contiguous(), b_seen, (b_row, b_col), block_bytes)
                rank = torch.empty(tcol.numel(), dtype=torch.int32, device=dev)
                ranked = torch.empty(B, dtype=torch.int32, device=dev)
                rank[s_entry], ranked[small] = part[0], part[1]
                rank[b_entry], ranked[big] = b_rank, b_ranked
                out = rank, ranked
    if out is None:
        out = _scored_ranks(model, r, users, seen, targets, block_bytes)
    return out


def _metric_names(cutoffs):
    names = []
    for K in cutoffs:
        names += [f"hr@{K}", f"recall@{K}", f"ndcg@{K}"]
    return names + ["mrr", "auc", "users"]


def _metrics_tensor(rank, rowptr, ranked, cutoffs):
    """The metrics as one float64 vector on rank's device, in the order of _metric_names; nothing is read back here."""
    dev = rank.device
    U = rowptr.numel() - 1
    f64 = torch.float64
    cnt = (rowptr[1:] - rowptr[:-1]).to(torch.int64)
    row = torch.repeat_interleave(torch.arange(U, device=dev), cnt.to(dev), output_size=rank.numel())
    r = rank.to(torch.int64)
    valid = r >= 0
    rz = torch.where(valid, r, torch.zeros_like(r))
    per_user = lambda v: torch.zeros(U, dtype=f64, device=dev).index_add_(0, row, v.to(f64))
    T = per_user(valid)
    has = T > 0
    n_users = has.sum().to(f64)
    Tz = torch.where(has, T, torch.ones_like(T))
    gain = 1.0 / torch.log2(rz.to(f64) + 2.0)
    maxK = max(cutoffs)
    ideal = torch.cumsum(1.0 / torch.log2(torch.arange(maxK, dtype=f64, device=dev) + 2.0), 0)    # ideal[i]: i + 1 hits on top
    mean = lambda v, m: torch.where(m, v, torch.zeros_like(v)).sum() / m.sum().to(f64)
    out = []
    for K in cutoffs:
        hit = valid & (r < K)
        hits = per_user(hit)
        dcg = per_user(torch.where(hit, gain, torch.zeros_like(gain)))
        idcg = ideal[(torch.clamp(T, max=K).to(torch.int64) - 1).clamp_min(0)]
        out += [mean((hits > 0).to(f64), has), mean(hits / Tz, has), mean(dcg / idcg, has)]
    big = torch.iinfo(torch.int64).max
    first = torch.full((U,), big, dtype=torch.int64, device=dev).scatter_reduce_(0, row, torch.where(valid, r, torch.full_like(r, big)),
                                                                                  "amin")
    out.append(mean(1.0 / (torch.where(has, first, torch.zeros_like(first)).to(f64) + 1.0), has))
    # sum_j (rank_j - j) over the user's valid ranks in ascending order, j = 0 .. T-1: the sum of the ranks minus T (T - 1) / 2
    inversions = per_user(rz) - T * (T - 1.0) / 2.0
    others = ranked.to(f64) - T
    auc_ok = has & (others > 0)
    out.append(mean(1.0 - inversions / torch.where(auc_ok, T * others, torch.ones_like(T)), auc_ok))
    out.append(n_users)
    return torch.stack(out)


def ranking_metrics(rank: torch.Tensor, targets_rowptr: torch.Tensor, ranked: torch.Tensor, cutoffs: Sequence[int] = (5, 10, 20)) -> dict:
    """HR@K, Recall@K, NDCG@K (for every K of ``cutoffs``), MRR and AUC of the ranks ``rank_of_items`` returns, as a dict of Python
    floats with keys ``hr@K``, ``recall@K``, ``ndcg@K``, ``mrr``, ``auc`` and ``users`` (the number of users averaged over).
    Computed in float64 on ``rank``'s device (CPU tensors work too); one host read.

    rank: (n_targets,) ranks, targets_rowptr: (U + 1,) the target CSR's row pointer, ranked: (U,) non-excluded columns per user.
    A user's valid targets are those with rank >= 0; T is their number; the means run over the users with T > 0.  Per user:
      hits@K = #{rank < K};  recall@K = hits@K / T;  hr@K = [hits@K > 0];
      ndcg@K = sum_{rank < K} 1 / log2(rank + 2)  /  sum_{i < min(T, K)} 1 / log2(i + 2);
      mrr    = 1 / (min rank + 1);
      auc    = 1 - sum_j (rank_j - j) / (T (ranked - T)) with the valid ranks ascending and j = 0 .. T-1: the share of (target,
               other column) pairs the model orders correctly; users with ranked == T are left out of its mean.
    The targets of a user must be unique (``held_out_items`` de-duplicates): a repeated target would count twice in T and share
    one rank.  With no user to average over a metric is nan."""
    cutoffs = [int(K) for K in cutoffs]
    if not cutoffs or min(cutoffs) < 1:
        raise ValueError("cutoffs must be positive")
    if rank.dim() != 1 or targets_rowptr.dim() != 1 or ranked.dim() != 1 or ranked.numel() != targets_rowptr.numel() - 1:
        raise ValueError("rank (n_targets,), targets_rowptr (U + 1,), ranked (U,)")
    dev = rank.device
    vals = _metrics_tensor(rank, targets_rowptr.to(dev), ranked.to(dev), cutoffs).tolist()      # the one host read
    return dict(zip(_metric_names(cutoffs), vals))


def eval_full_ranking(model, user_ids: torch.Tensor, targets, exclude=None, cutoffs: Sequence[int] = (5, 10, 20), **route) -> dict:
    """``ranking_metrics`` of ``rank_of_items(model, user_ids, targets, exclude=exclude, **route)`` (route: item_ids, graph, fused,
    max_targets, block_bytes, profiles).  The metrics, the out-of-range flag and the target overflow flag come back in one host read; a set
    flag raises (IndexError / OverflowError) as ``native.check_oob`` / ``native.check_rank_overflow`` do."""
    cutoffs = [int(K) for K in cutoffs]
    rank, ranked = rank_of_items(model, user_ids, targets, exclude=exclude, **route)
    dev = rank.device
    oob, over = native._oob_flag(dev), native._rank_overflow_flag(dev)
    vals = torch.cat([_metrics_tensor(rank, targets[0].to(dev), ranked, cutoffs), oob.to(torch.float64), over.to(torch.float64)]).tolist()
    if vals[-2] != 0:
        oob.zero_()
        raise IndexError("index out of range in an embedding gather")
    if vals[-1] != 0:
        over.zero_()
        raise OverflowError("a user has more targets than the max_targets the rank call was given")
    return dict(zip(_metric_names(cutoffs), vals[:-2]))


def held_out_items(samples, user_positions, item_positions, device=None):
    """The users of a test DataFrame and their held-out items: ``(user_ids (U,) int64, (rowptr (U + 1) int64, col int32))`` for
    ``rank_of_items``.  samples: a DataFrame with ``userId`` and ``movieId`` columns; user_positions / item_positions: the id ->
    position maps of the model's provider (``IndexProvider.get_user_profile`` / ``get_item_profile``;
    ``IndexGraphProvider.get_user_nodeID`` / ``get_item_nodeID``), as ``seen_items`` uses a graph's node positions.  Users come in
    ascending position, each with its distinct items in ascending position (a pair listed twice counts once).  Built on the host;
    ``device`` moves the three tensors."""
    u = np.asarray(user_positions(samples["userId"].values), dtype=np.int64)
    i = np.asarray(item_positions(samples["movieId"].values), dtype=np.int64)
    pairs = np.unique(np.stack([u, i], 1), axis=0) if len(u) else np.zeros((0, 2), dtype=np.int64)
    users, counts = np.unique(pairs[:, 0], return_counts=True)
    rowptr = np.zeros(len(users) + 1, dtype=np.int64)
    np.cumsum(counts, out=rowptr[1:])
    out = torch.from_numpy(users), (torch.from_numpy(rowptr), torch.from_numpy(pairs[:, 1].astype(np.int32)))
    if device is not None:
        out = out[0].to(device), (out[1][0].to(device), out[1][1].to(device))
    return out


# ---------------------------------------------------------------------------------------- beyond accuracy: diversity and coverage
def _lists(positions, counts, who):
    if not torch.is_tensor(positions) or positions.dtype != torch.int64 or positions.dim() != 2:
        raise ValueError(f"{who}: positions must be a (B, k) int64 tensor of item positions")
    if counts is not None and (not torch.is_tensor(counts) or counts.dim() != 1 or counts.numel() != positions.shape[0]
                               or counts.dtype not in (torch.int32, torch.int64)):
        raise ValueError(f"{who}: counts must be a ({positions.shape[0]},) int32 tensor")
    used = positions >= 0
    if counts is not None:
        used = used & (torch.arange(positions.shape[1], device=positions.device)[None, :] < counts[:, None])
    return used


def intra_list_diversity(positions: torch.Tensor, counts: Optional[torch.Tensor], item_vectors: torch.Tensor) -> torch.Tensor:
    """Intra-list diversity of recommendation lists: per list the mean over its unordered pairs of items of ``1 - sim``, ``sim`` the
    dot product of the two items' rows of ``item_vectors`` (unit rows: one minus the cosine).  positions (B, k) int64 and counts (B,)
    int32 (or None) as ``top_k_items`` / ``diversify_top_k`` return them: slots past ``counts`` and slots holding -1 are not part of
    a list.  Returns (B,) fp32 on the lists' device, NaN for a list of fewer than two items; summed in float64.  No host sync."""
    used = _lists(positions, counts, "intra_list_diversity")
    if not torch.is_tensor(item_vectors) or item_vectors.dim() != 2 or not item_vectors.is_floating_point():
        raise ValueError("intra_list_diversity: item_vectors must be a (n_items, D) floating-point tensor")
    with torch.no_grad():
        rows = item_vectors[positions.clamp_min(0)].to(torch.float64)                      # (B, k, D)
        gram = torch.bmm(rows, rows.transpose(1, 2))
        pair = (used[:, :, None] & used[:, None, :]).triu(diagonal=1)
        total = ((1.0 - gram) * pair).sum(dim=(1, 2))
        return (total / pair.sum(dim=(1, 2)).to(torch.float64)).to(torch.float32)          # 0 / 0: NaN under two items


def catalogue_coverage(positions: torch.Tensor, counts: Optional[torch.Tensor], n_items: int) -> torch.Tensor:
    """Catalogue coverage of recommendation lists: the number of distinct item positions in all lists together, divided by
    ``n_items``.  positions / counts as in ``intra_list_diversity``; a position outside ``[0, n_items)`` counts for nothing.  Returns a
    float64 scalar on the lists' device.  No host sync."""
    used = _lists(positions, counts, "catalogue_coverage")
    if isinstance(n_items, bool) or not isinstance(n_items, (int, np.integer)) or n_items < 1:
        raise ValueError(f"catalogue_coverage: n_items = {n_items!r} is not a positive int")
    with torch.no_grad():
        used = used & (positions < n_items)
        hit = torch.zeros(int(n_items) + 1, dtype=torch.int64, device=positions.device)
        hit[torch.where(used, positions, torch.full_like(positions, int(n_items))).reshape(-1)] = 1    # slot n_items: the unused
        return hit[:int(n_items)].sum().to(torch.float64) / float(n_items)
