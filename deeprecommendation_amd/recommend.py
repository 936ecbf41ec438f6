"""Top-K recommendation on the device: the library function behind the reference's web backend (webapp/backend.py:78-121).

``top_k_items``        BasicNCF / MF (index providers), GraphNCF and AttentionNCF (``profiles=``): every listed user against every item (or a subset), scored
                       block by block through the model's HIP scoring path and ranked by ncf_topk_rows — or scored and ranked in
                       one pass (no score matrix) by ncf_dot_topk for a dot-product readout and by ncf_mlp_topk for an MLP
                       readout.  Results stay on the device.
                       A BasicNCF with content attached (``set_content``) ranks the rows of its item table like a one-hot model.
``content_cosine_top_k`` / ``content_cosine_ranks``
                       the reference's content-based baseline: cosine of a user's fixed profile and an item's feature row.
``item_knn_top_k`` / ``item_knn_ranks``
                       the neighbourhood baseline: a fitted ``baselines.ItemKNN`` scored over the catalogue (ncf_knn_scores) and ranked.
``ease_top_k`` / ``ease_ranks``
                       the closed-form item-item baseline: a fitted ``baselines.EASE`` scored over the catalogue (ncf_ease_scores) and ranked.
``slim_top_k`` / ``slim_ranks``
                       the sparse item-item baseline: a fitted ``baselines.SLIM`` scored and ranked through the same scorer.
``diversify_top_k``    greedy MMR re-ranking of the pools those two return (native.mmr_rerank, one launch): relevance traded against the
                       similarity to what is already in the list.  ``item_vectors`` gives a model's own item space for it.
``seen_items``         the exclusion lists of a graph's users (their training interactions) for top_k_items.
``rated_exclusion``    the same for an AttentionNCF's users: the items each listed user rated.
``explain_items``      AttentionNCF: the reasons behind winners of many users at once (which rated items carry the attention), from the
                       shared logit table; the batch counterpart of recommend_for_user's ``because`` / ``attention`` columns.
``recommend_for_user`` AttentionNCF: one user given as a Series of ratings against a catalogue, with the reference's arguments,
                       threshold rule and DataFrame columns (imdbID, score, because, attention).  Only k scores, k ids and the k
                       winners' attention rows cross to the host.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import native
from .neural_collaborative_filtering.models.attention_ncf import RowsOf, SparseRatings
from .neural_collaborative_filtering.util import require_gpu

# bound of one score block of top_k_items: scores (4 B) + the two int64 position columns (16 B) per (user, item) pair
BLOCK_BYTES = 256 << 20
_PAIR_BYTES = 4 + 16


def _model_device(model) -> torch.device:
    return next(model.parameters()).device


def _eval_only(model):
    if model.training:
        raise RuntimeError("recommendations are computed in eval mode: call model.eval() first")


def _graph_model(model) -> bool:
    from .neural_collaborative_filtering.models.gnn_ncf import GraphNCF
    return isinstance(model, GraphNCF)


def _dot_readout(model) -> bool:
    from .neural_collaborative_filtering.models.mf import MF
    return isinstance(model, MF) or (_graph_model(model) and model.MLP is None)


class _RankedList(NamedTuple):
    """What top_k_items and rank_of_items rank, resolved from their shared arguments (_resolve_ranked)."""
    graph: object                # the GraphData on the device; None for a model without one
    users: torch.Tensor          # (B,) int64 user positions, contiguous
    items: torch.Tensor          # (I,) int64 item positions: the ranked list's columns
    all_items: bool              # the list is every item of the model in position order (item_ids not given)
    n_items: int
    seen: Optional[tuple]        # the exclusion CSR (rowptr (B + 1) int64, col int32), or None
    B: int
    I: int
    profiles: Optional[tuple] = None   # (item_features, ratings) of an AttentionNCF; None for every other model
    table: Optional[bool] = None       # AttentionNCF: catalogue_scores' route (fused=None / True / False)


def _csr(pair, B, what):
    """A per-user CSR argument ``(rowptr (B + 1), col)`` as the kernels take it: int64 / int32, contiguous."""
    rowptr, col = pair
    require_gpu(rowptr, col)
    if rowptr.dim() != 1 or col.dim() != 1 or rowptr.numel() != B + 1:
        raise ValueError(f"{what} = (rowptr ({B + 1},) int64, col int32): rowptr has {rowptr.numel()} entries")
    return rowptr.to(torch.int64).contiguous(), col.to(torch.int32).contiguous()


def _attention_model(model) -> bool:
    from .neural_collaborative_filtering.models.attention_ncf import AttentionNCF
    return isinstance(model, AttentionNCF)


def _resolve_attention(model, user_ids, item_ids, exclude, profiles, fused) -> _RankedList:
    """_resolve_ranked for an AttentionNCF: ``profiles = (item_features (I_c, F), ratings)``, users = rows of ``ratings``.  Every
    refusal that needs no device comes before the first that does."""
    if not (isinstance(profiles, (tuple, list)) and len(profiles) == 2 and torch.is_tensor(profiles[0]) and profiles[0].dim() == 2
            and all(hasattr(profiles[1], a) for a in ("rowptr", "col", "val", "num_items"))):
        raise ValueError("profiles = (item_features (I_c, F) tensor, ratings SparseRatings over the catalogue's positions)")
    item_features, ratings = profiles
    if not isinstance(ratings, SparseRatings):       # a provider's device state: every user's rated set as one CSR
        ratings = SparseRatings(ratings.rowptr, ratings.col, ratings.val, ratings.num_items)
    if user_ids.dtype != torch.int64 or user_ids.dim() != 1:
        raise ValueError("user_ids must be a 1-D int64 tensor of user positions")
    if item_ids is not None and (item_ids.dtype != torch.int64 or item_ids.dim() != 1):
        raise ValueError("item_ids must be a 1-D int64 tensor of item positions")
    if ratings.num_items != item_features.shape[0]:
        raise ValueError(f"ratings has {ratings.num_items} columns, the catalogue {item_features.shape[0]} rows")
    n_items = item_features.shape[0]
    model.cross_route(n_items, fused)               # fused=True outside the table route's limits: ValueError
    require_gpu(user_ids, item_ids, item_features, ratings.rowptr)
    dev = user_ids.device
    items = torch.arange(n_items, dtype=torch.int64, device=dev) if item_ids is None else item_ids.contiguous()
    B = user_ids.numel()
    seen = None if exclude is None else _csr(exclude, B, "exclude")
    return _RankedList(None, user_ids.contiguous(), items, item_ids is None, n_items, seen, B, items.numel(), (item_features, ratings), fused)


def _resolve_ranked(model, user_ids, item_ids, exclude, graph, profiles=None, fused=None) -> _RankedList:
    """The checks top_k_items and rank_of_items make on the arguments they share, and the ranked list those arguments name."""
    _eval_only(model)
    if _attention_model(model):
        if profiles is None:
            raise ValueError("an AttentionNCF ranks items for users given by their ratings: pass profiles=(item_features, ratings)")
        if graph is not None:
            raise ValueError(f"graph= is only taken by a GraphNCF, not by {type(model).__name__}")
        return _resolve_attention(model, user_ids, item_ids, exclude, profiles, fused)
    if profiles is not None:
        raise ValueError(f"profiles= is only taken by an AttentionNCF, not by {type(model).__name__}")
    require_gpu(user_ids)
    dev = user_ids.device
    if user_ids.dtype != torch.int64 or user_ids.dim() != 1:
        raise ValueError("user_ids must be a 1-D int64 tensor of user positions")
    is_graph = _graph_model(model)
    if is_graph and graph is None:
        raise ValueError("a GraphNCF ranks items on a graph: pass graph=")
    if not is_graph and graph is not None:
        raise ValueError(f"graph= is only taken by a GraphNCF, not by {type(model).__name__}")
    if is_graph:
        graph = graph.to(dev)
        n_items = graph.num_items
    else:
        n_items = model.num_items       # a BasicNCF with content attached: the rows of its item table, not the feature width
    if item_ids is None:
        items = torch.arange(n_items, dtype=torch.int64, device=dev)
    else:
        require_gpu(item_ids)
        if item_ids.dtype != torch.int64 or item_ids.dim() != 1:
            raise ValueError("item_ids must be a 1-D int64 tensor of item positions")
        items = item_ids.contiguous()
    B = user_ids.numel()
    seen = None if exclude is None else _csr(exclude, B, "exclude")
    return _RankedList(graph, user_ids.contiguous(), items, item_ids is None, n_items, seen, B, items.numel())


def _user_blocks(n_users, block_bytes, row_bytes, max_rows=None):
    """Yields ``(b0, b1)``: the users in consecutive blocks of as many rows of ``row_bytes`` as fit ``block_bytes`` (at least one, at
    most ``max_rows``)."""
    rows_per_block = max(1, int(block_bytes) // max(1, row_bytes))
    if max_rows is not None:
        rows_per_block = min(rows_per_block, max_rows)
    for b0 in range(0, n_users, rows_per_block):
        yield b0, min(n_users, b0 + rows_per_block)


def _position_lists(**lists):
    for what, t in lists.items():
        if t is not None and (not torch.is_tensor(t) or t.dtype != torch.int64 or t.dim() != 1):
            raise ValueError(f"{what} must be a 1-D int64 tensor of positions")


def _check_k(k):
    if not 1 <= int(k) <= native.TOPK_MAX_K:
        raise ValueError(f"k = {k} is outside 1 .. {native.TOPK_MAX_K}")


def _item_positions(idx, items):
    """Columns of the ranked list (-1: an unused slot) as int64 item positions; ``items`` None: the columns are the positions."""
    pos = idx.to(torch.int64)
    return pos if items is None else torch.where(pos >= 0, items[pos.clamp_min(0)], pos)


def _select_blocks(blocks, B, k, exclude, items, dev):
    """The score-then-select tail of every top-K entry point: ``k`` is checked, then the score blocks ``(b0, b1, scores (b1 - b0,
    I))`` of ``blocks`` (a generator: its own checks run after these) are ranked one by one with native.topk_rows, skipping ``exclude``
    (a per-user CSR over all ``B`` users, or None), joined, and mapped through ``items`` (_item_positions).  No block (B = 0): empty
    results on ``dev``."""
    _check_k(k)
    seen = None if exclude is None else _csr(exclude, B, "exclude")
    # the kernel reads seen_col[rowptr[r] ..]: a slice of rowptr indexes the whole col array, no rebasing
    with torch.no_grad():
        outs = [native.topk_rows(scores, int(k), None if seen is None else (seen[0][b0:b1 + 1], seen[1])) for b0, b1, scores in blocks]
    if not outs:
        return (torch.empty((0, int(k)), dtype=torch.float32, device=dev), torch.empty((0, int(k)), dtype=torch.int64, device=dev),
                torch.empty(0, dtype=torch.int32, device=dev))
    s, idx, cnt = (torch.cat([o[j] for o in outs]) if len(outs) != 1 else outs[0][j] for j in range(3))
    return s, _item_positions(idx, items), cnt


def _rank_blocks(blocks, B, targets, exclude):
    """The score-then-rank tail of every ranks entry point: the targets (a per-user CSR over all ``B`` users) of each score block of
    ``blocks`` are ranked in its score rows with native.rank_rows, skipping ``exclude``.  Returns ``(rank (n_targets,) int32, ranked
    (B,) int32)``; no block (B = 0): ``ranked`` is empty."""
    trow, tcol = _csr(targets, B, "targets")
    seen = None if exclude is None else _csr(exclude, B, "exclude")
    rank = torch.empty(tcol.numel(), dtype=torch.int32, device=tcol.device)
    # the kernels read col[rowptr[r] ..] and write rank[rowptr[r] ..]: a slice of rowptr indexes the whole arrays
    with torch.no_grad():
        ranked = [native.rank_rows(scores, (trow[b0:b1 + 1], tcol), None if seen is None else (seen[0][b0:b1 + 1], seen[1]), rank=rank)[1]
                  for b0, b1, scores in blocks]
    if not ranked:
        return rank, torch.empty(0, dtype=torch.int32, device=tcol.device)
    return rank, (torch.cat(ranked) if len(ranked) != 1 else ranked[0])


def _csr_take(start, count):
    """The CSR made of the entry spans ``[start[i], start[i] + count[i])`` of another, in the listed order (a span may be empty or
    listed twice): ``(rowptr (n + 1) int64, entry)`` with ``entry`` = the place of each kept entry in the source.  Sizes its result on
    the host (one read)."""
    n, dev = start.numel(), start.device
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(count, 0, out=rowptr[1:])
    row = torch.repeat_interleave(torch.arange(n, device=dev), count)
    return rowptr, start[row] + torch.arange(row.numel(), device=dev) - rowptr[row]


def _score_blocks(model, r: _RankedList, users, block_bytes):
    """Yields ``(b0, b1, scores (b1 - b0, I))``: the users scored against the ranked list through the model, in blocks of rows
    whose (user, item) score block stays under ``block_bytes``."""
    if r.profiles is not None:           # AttentionNCF: the model blocks its own user_emb rows (4 * UE bytes per pair)
        yield from model.catalogue_score_blocks(r.profiles[0], r.profiles[1], users, None if r.all_items else r.items, r.table, block_bytes)
        return
    score = (lambda u, i: model(r.graph, u, i)) if r.graph is not None else model
    for b0, b1 in _user_blocks(users.numel(), block_bytes, r.I * _PAIR_BYTES):
        with torch.no_grad():
            scores = score(users[b0:b1].repeat_interleave(r.I), r.items.repeat(b1 - b0)).view(b1 - b0, r.I)
        yield b0, b1, scores                  # outside the with: a suspended generator must not hold the grad mode


def top_k_items(model, user_ids: torch.Tensor, k: int, item_ids: Optional[torch.Tensor] = None,
                exclude: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, block_bytes: int = BLOCK_BYTES, *, graph=None,
                fused: Optional[bool] = None, profiles=None):
    """The ``k`` best items of every user in ``user_ids`` for a BasicNCF / MF / NeuMF / GraphNCF model (int64 position inputs).

    user_ids: (B,) int64 user positions on the GPU — for a GraphNCF node positions as in ``GraphNCF.forward`` (users come after
    the ``graph.num_items`` items).  item_ids: optional (I,) int64 item positions to rank (default: every item of the model; for
    a GraphNCF every item node ``0 .. graph.num_items - 1``).  exclude: optional per-user CSR ``(rowptr (B + 1) int64, col
    int32)`` of columns of the ranked list to skip (with ``item_ids`` absent, columns are item positions) — typically each
    user's training ratings (``seen_items`` builds it from a graph).  graph: the GraphData a GraphNCF is evaluated on; required
    for a GraphNCF and refused for any other model.
    fused: how the scores are ranked.  ``None``: GraphNCF-dot through the fused dot-product score-and-select kernel
    (``native.dot_topk``), and an MLP readout (BasicNCF, GraphNCF with ``use_dot_product=False``) through the fused MLP
    score-and-select kernel (``native.mlp_topk``; a NeuMF through the same waves with its GMF term, ``native.neumf_topk``), none of
    which writes a score matrix; MF score-then-select.  ``True``: the
    fused dot-product kernel for MF too (refused for a model with an MLP readout); ``False``: score-then-select everywhere.  All
    routes give the same bits.  Where a fused kernel's limits do not hold it falls back to score-then-select: k <= 128 for both;
    width <= 256 for the dot kernel; for the MLP kernel fp32 scoring, no folded first layer and an MLP shape with an
    ``ncf_score_fused`` instance; for a NeuMF also at most two hidden layers and ``mf_dim`` a multiple of 8 up to 128.
    profiles: ``(item_features (I_c, F), ratings)`` for an AttentionNCF — required for that model and refused for any other.  The
    catalogue is both the candidate list and the rated-item list; ``ratings`` is a SparseRatings whose rows are users and whose
    columns are catalogue positions (``SparseDynamicProvider.device_state``), ``user_ids`` are rows of it, ``item_ids`` / ``exclude``
    keep their meaning (``rated_exclusion`` builds the users' rated items as ``exclude``).  ``fused`` then picks the route of
    ``AttentionNCF.catalogue_scores``: ``None`` / ``True`` / ``False`` = its ``table=``; the score blocks are ranked by
    ``native.topk_rows`` on either route (there is no fused score-and-select kernel for this model).
    Returns ``(scores (B, k) fp32, item_positions (B, k) int64, counts (B,) int32)`` on the device, each row in descending score
    order (ties: lower column first; NaN last); slots past ``counts`` hold position -1 and score -inf.  Score-then-select scores
    the users in blocks of rows whose (user, item) score block stays under ``block_bytes``; nothing synchronises with the host.
    An empty ``user_ids`` gives ``(0, k)``, ``(0, k)`` and ``(0,)`` results on every route."""
    r = _resolve_ranked(model, user_ids, item_ids, exclude, graph, profiles, fused)
    if r.profiles is not None:
        fused = False                     # no fused score-and-select kernel for this model: catalogue_scores, then ncf_topk_rows
    if fused and not _dot_readout(model):
        raise ValueError(f"fused=True needs a dot-product readout; {type(model).__name__} here scores through an MLP")
    if fused and getattr(model, "scoring_dtype", torch.float32) != torch.float32:
        raise ValueError("fused=True takes fp32 tables: the model scores in " + str(model.scoring_dtype))
    _check_k(k)
    out = None
    if bool(fused) if fused is not None else (r.graph is not None and _dot_readout(model)):
        out = _fused_top_k(model, r, int(k))
    elif fused is None and not _dot_readout(model):
        out = _fused_mlp_top_k(model, r, int(k))
    items = None if r.all_items else r.items
    if out is None:
        return _select_blocks(_score_blocks(model, r, r.users, block_bytes), r.B, k, r.seen, items, r.users.device)
    s, idx, cnt = out
    return s, _item_positions(idx, items), cnt


def _fused_top_k(model, r: _RankedList, k):
    """native.dot_topk over the model's (user table, item table); None where the fused kernel's limits do not hold (the caller
    then scores and selects, which gives the same bits)."""
    if k > native.DOT_TOPK_MAX_K:
        return None
    with torch.no_grad():
        user_tab, item_tab, ids = _fused_tables(model, r, model._refresh())
        if user_tab.shape[1] > native.DOT_TOPK_MAX_D:
            return None
        return native.dot_topk(user_tab, r.users, item_tab, ids, k, r.seen)


def _neumf_model(model) -> bool:
    from .neural_collaborative_filtering.models.neumf import NeuMF
    return isinstance(model, NeuMF)


def _mlp_operands(model, r: _RankedList, users):
    """``(tabA, idxA, tabB, idxB, packed, user_first, gmf)`` of a fused MLP readout over ``users`` and the ranked list — BasicNCF:
    cat(user table, item table), the users first; GraphNCF: cat(item node rows, user node rows) of the propagated table, the items
    first; NeuMF: its tower like a BasicNCF, with ``gmf`` = (GMF user table, GMF item table, w) for the NeuMF kernels (None for
    the others).  None where no fused MLP kernel applies: non-fp32 scoring, a folded first layer, no packed MLP, a NeuMF shape
    outside its kernels' limits."""
    if getattr(model, "scoring_dtype", torch.float32) != torch.float32 or model.fold_first_layer:
        return None
    cache = model._refresh()
    if _neumf_model(model):
        ops = model.kernel_operands(cache)
        if ops is None:
            return None
        user_tab, item_tab, gmf_user, gmf_item, packed, w = ops
        return user_tab, users, item_tab, None if r.all_items else r.items, packed, True, (gmf_user, gmf_item, w)
    packed = model._packed_mlp("MLP", cache)
    if packed is None:
        return None
    user_tab, item_tab, ids = _fused_tables(model, r, cache)
    if r.graph is None:
        return user_tab, users, item_tab, ids, packed, True, None
    return item_tab, ids, user_tab, users, packed, False, None


def _fused_mlp_top_k(model, r: _RankedList, k):
    """native.mlp_topk (a NeuMF: native.neumf_topk) over the model's MLP readout; None where the fused kernel does not apply
    (_mlp_operands, an MLP shape without a fused instance, k > 128); the caller then scores and selects, which gives the same bits."""
    if k > native.MLP_TOPK_MAX_K:
        return None
    with torch.no_grad():
        ops = _mlp_operands(model, r, r.users)
        if ops is None:
            return None
        tabA, idxA, tabB, idxB, packed, user_first, gmf = ops
        if not native.mlp_topk_supported(packed, tabA.shape[1], tabB.shape[1], k):
            return None
        if gmf is not None:
            return native.neumf_topk(tabA, idxA, tabB, idxB, gmf[0], gmf[1], packed, gmf[2], k, r.seen)
        return native.mlp_topk(tabA, idxA, tabB, idxB, packed, k, r.seen, user_first=user_first)


def _fused_tables(model, r: _RankedList, cache):
    """(user table, item table, item ids or None) of a fused route: a GraphNCF's propagated node table (its first n_items rows are
    the item nodes: all items are ranked in place, without an id list), else the model's user and item embedding tables."""
    if r.graph is not None:
        combined = model.propagate_all(r.graph, cache)
        return (combined, combined[:r.n_items], None) if r.all_items else (combined, combined, r.items)
    user_tab = model._table("user", model.user_embeddings[0], cache)
    item_tab = model._table("item", model.item_embeddings[0], cache)
    return user_tab, item_tab, None if r.all_items else r.items


def seen_items(graph, user_ids: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The exclusion CSR ``(rowptr (B + 1) int64, col int32)`` of each listed user's training interactions — the item ends of
    the graph's ``user2item`` edges whose source is that user — in the column space of ``top_k_items``' default item list (item
    positions ``0 .. graph.num_items - 1``).  user_ids: (B,) int64 node positions on the GPU, as ``top_k_items`` takes them.
    Built on the device with torch ops; a row lists its items in edge order (duplicate edges repeat)."""
    require_gpu(user_ids)
    if user_ids.dtype != torch.int64 or user_ids.dim() != 1:
        raise ValueError("user_ids must be a 1-D int64 tensor of user node positions")
    dev = user_ids.device
    ei = graph.user2item_edge_index.to(dev)
    src, dst = ei[0].to(torch.int64), ei[1].to(torch.int64)
    order = torch.argsort(src, stable=True)
    s_src, s_dst = src[order], dst[order]
    lo = torch.searchsorted(s_src, user_ids)
    rowptr, pos = _csr_take(lo, torch.searchsorted(s_src, user_ids, right=True) - lo)
    return rowptr, s_dst[pos].to(torch.int32)


def rated_exclusion(ratings: SparseRatings, user_ids: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The exclusion CSR ``(rowptr (B + 1) int64, col int32)`` of each listed user's rated items — the counterpart of ``seen_items``
    for an AttentionNCF's ``profiles=`` (the web backend's ``ignore_seen=True``), in the column space of ``top_k_items``' default item
    list (catalogue positions).  user_ids: (B,) int64 rows of ``ratings`` on the GPU.  Built on the device with torch ops; a row
    lists its items in the order of ``ratings`` (a masked entry, outside the catalogue, excludes nothing)."""
    require_gpu(user_ids, ratings.rowptr, ratings.col)
    if user_ids.dtype != torch.int64 or user_ids.dim() != 1:
        raise ValueError("user_ids must be a 1-D int64 tensor of rows of ratings")
    lo = ratings.rowptr[user_ids]
    rowptr, pos = _csr_take(lo, ratings.rowptr[user_ids + 1] - lo)
    return rowptr, ratings.col[pos].to(torch.int32)


# ---------------------------------------------------------------------------------------- content-based baseline
def _cosine_blocks(user_profiles, item_features, user_ids, item_ids, block_bytes):
    """Yields ``(b0, b1, cosines (b1 - b0, I))`` of the listed users' profiles against the ranked list's feature rows: both sides
    L2-normalised by rows (ncf_l2_normalize_rows: a zero row stays zero), then one Linear launch per block of users."""
    for t, what in ((user_profiles, "user_profiles"), (item_features, "item_features")):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 2:
            raise ValueError(f"{what} must be a 2-D float32 tensor")
    if user_profiles.shape[1] != item_features.shape[1]:
        raise ValueError(f"user_profiles has {user_profiles.shape[1]} columns, item_features {item_features.shape[1]}")
    _position_lists(user_ids=user_ids, item_ids=item_ids)
    require_gpu(user_profiles, item_features, user_ids, item_ids)
    with torch.no_grad():
        items = native.l2_normalize_rows(item_features if item_ids is None else native.gather_concat(item_features, item_ids.contiguous()))
    users = user_ids.contiguous()
    for b0, b1 in _user_blocks(users.numel(), block_bytes, items.shape[0] * 4):
        with torch.no_grad():
            prof = native.l2_normalize_rows(native.gather_concat(user_profiles, users[b0:b1]))
            scores = native.linear(prof, items, None)
        yield b0, b1, scores                  # outside the with: a suspended generator must not hold the grad mode


def content_cosine_top_k(user_profiles: torch.Tensor, item_features: torch.Tensor, user_ids: torch.Tensor, k: int,
                         item_ids: Optional[torch.Tensor] = None, exclude: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                         block_bytes: int = BLOCK_BYTES):
    """The reference's content-based baseline (contentbased_baseline.py) on the device: the ``k`` items whose feature rows have the
    largest cosine with each listed user's fixed profile.  user_profiles (U, F) / item_features (I, F): fp32 device tables
    (``SparseDynamicProvider.user_profiles``, ``ContentIndexProvider.content``); user_ids, item_ids, exclude, block_bytes and the
    returned ``(scores (B, k), item_positions (B, k) int64, counts (B,) int32)`` as in ``top_k_items``.  A user whose profile is all
    zeros (no ratings) scores 0 against every item, as the reference leaves it, and so gets the first ``k`` columns."""
    return _select_blocks(_cosine_blocks(user_profiles, item_features, user_ids, item_ids, block_bytes), user_ids.numel(), k, exclude,
                          item_ids, user_profiles.device)


def content_cosine_ranks(user_profiles: torch.Tensor, item_features: torch.Tensor, user_ids: torch.Tensor,
                         targets: Tuple[torch.Tensor, torch.Tensor], item_ids: Optional[torch.Tensor] = None,
                         exclude: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, block_bytes: int = BLOCK_BYTES):
    """The ranks twin of ``content_cosine_top_k``: ``(rank (n_targets,) int32, ranked (B,) int32)`` of each listed user's held-out
    items under the baseline's cosines, with the meaning ``rank_of_items`` gives them (``ranking_metrics`` takes them as they are)."""
    return _rank_blocks(_cosine_blocks(user_profiles, item_features, user_ids, item_ids, block_bytes), user_ids.numel(), targets, exclude)


# ---------------------------------------------------------------------------------------- neighbourhood baseline
def _knn_blocks(model, ratings, user_ids, item_ids, block_bytes):
    """Yields ``(b0, b1, scores (b1 - b0, I))`` of the listed rows of ``ratings`` under a fitted ``baselines.ItemKNN``: one
    ncf_knn_scores launch per block of users over the whole catalogue, the ranked list's columns gathered from it."""
    _position_lists(user_ids=user_ids, item_ids=item_ids)
    model._fitted()
    require_gpu(user_ids, item_ids)
    users = user_ids.contiguous()
    for b0, b1 in _user_blocks(users.numel(), block_bytes, model.num_items_ * 4, native.KNN_MAX_ROWS):
        scores = model.scores(ratings, users[b0:b1])
        yield b0, b1, scores if item_ids is None else scores.index_select(1, item_ids)


def item_knn_top_k(model, ratings, user_ids: torch.Tensor, k: int, item_ids: Optional[torch.Tensor] = None,
                   exclude: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, block_bytes: int = BLOCK_BYTES):
    """The neighbourhood baseline's recommendations: the ``k`` items with the largest ItemKNN score for each listed user.  model: a
    fitted ``baselines.ItemKNN``; ratings: the CSR the users' rows are read from (a SparseRatings or (rowptr, col, val); not
    necessarily the fitted one); user_ids: (B,) int64 rows of it; item_ids, exclude, block_bytes and the returned ``(scores (B, k),
    item_positions (B, k) int64, counts (B,) int32)`` as in ``top_k_items`` (``rated_exclusion(ratings, user_ids)`` leaves out what
    a user rated)."""
    model._fitted()
    return _select_blocks(_knn_blocks(model, ratings, user_ids, item_ids, block_bytes), user_ids.numel(), k, exclude, item_ids,
                          user_ids.device)


def item_knn_ranks(model, ratings, user_ids: torch.Tensor, targets: Tuple[torch.Tensor, torch.Tensor],
                   item_ids: Optional[torch.Tensor] = None, exclude: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                   block_bytes: int = BLOCK_BYTES):
    """The ranks twin of ``item_knn_top_k``: ``(rank (n_targets,) int32, ranked (B,) int32)`` of each listed user's held-out items
    under the ItemKNN scores, with the meaning ``rank_of_items`` gives them (``ranking_metrics`` takes them as they are)."""
    model._fitted()
    return _rank_blocks(_knn_blocks(model, ratings, user_ids, item_ids, block_bytes), user_ids.numel(), targets, exclude)


# ---------------------------------------------------------------------------------------- EASE and SLIM baselines
def _item_item_blocks(model, ratings, user_ids, item_ids, block_bytes):
    """Yields ``(b0, b1, scores (b1 - b0, I))`` of the listed rows of ``ratings`` under a fitted model with a dense item-item matrix
    (``baselines.EASE``, ``baselines.SLIM``: ``_fitted()``, ``num_items_`` and ``scores``): one ncf_ease_scores launch per block of
    users over the whole catalogue, the ranked list's columns gathered from it."""
    _position_lists(user_ids=user_ids, item_ids=item_ids)
    model._fitted()
    require_gpu(user_ids, item_ids)
    users = user_ids.contiguous()
    for b0, b1 in _user_blocks(users.numel(), block_bytes, model.num_items_ * 4, native.EASE_MAX_ROWS):
        scores = model.scores(ratings, users[b0:b1])
        yield b0, b1, scores if item_ids is None else scores.index_select(1, item_ids)


def ease_top_k(model, ratings, user_ids: torch.Tensor, k: int, item_ids: Optional[torch.Tensor] = None,
               exclude: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, block_bytes: int = BLOCK_BYTES):
    """The EASE baseline's recommendations: the ``k`` items with the largest EASE score for each listed user.  model: a fitted
    ``baselines.EASE``; every other argument and the returned ``(scores (B, k), item_positions (B, k) int64, counts (B,) int32)`` as in
    ``item_knn_top_k``."""
    model._fitted()
    return _select_blocks(_item_item_blocks(model, ratings, user_ids, item_ids, block_bytes), user_ids.numel(), k, exclude, item_ids,
                          user_ids.device)


def ease_ranks(model, ratings, user_ids: torch.Tensor, targets: Tuple[torch.Tensor, torch.Tensor],
               item_ids: Optional[torch.Tensor] = None, exclude: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
               block_bytes: int = BLOCK_BYTES):
    """The ranks twin of ``ease_top_k``: ``(rank (n_targets,) int32, ranked (B,) int32)`` of each listed user's held-out items under
    the EASE scores, with the meaning ``rank_of_items`` gives them (``ranking_metrics`` takes them as they are)."""
    model._fitted()
    return _rank_blocks(_item_item_blocks(model, ratings, user_ids, item_ids, block_bytes), user_ids.numel(), targets, exclude)


def slim_top_k(model, ratings, user_ids: torch.Tensor, k: int, item_ids: Optional[torch.Tensor] = None,
               exclude: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, block_bytes: int = BLOCK_BYTES):
    """The SLIM baseline's recommendations: the ``k`` items with the largest SLIM score for each listed user.  model: a fitted
    ``baselines.SLIM``; every other argument and the returned ``(scores (B, k), item_positions (B, k) int64, counts (B,) int32)`` as in
    ``item_knn_top_k``."""
    model._fitted()
    return _select_blocks(_item_item_blocks(model, ratings, user_ids, item_ids, block_bytes), user_ids.numel(), k, exclude, item_ids,
                          user_ids.device)


def slim_ranks(model, ratings, user_ids: torch.Tensor, targets: Tuple[torch.Tensor, torch.Tensor],
               item_ids: Optional[torch.Tensor] = None, exclude: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
               block_bytes: int = BLOCK_BYTES):
    """The ranks twin of ``slim_top_k``: ``(rank (n_targets,) int32, ranked (B,) int32)`` of each listed user's held-out items under
    the SLIM scores, with the meaning ``rank_of_items`` gives them (``ranking_metrics`` takes them as they are)."""
    model._fitted()
    return _rank_blocks(_item_item_blocks(model, ratings, user_ids, item_ids, block_bytes), user_ids.numel(), targets, exclude)


# ---------------------------------------------------------------------------------------- diversified top-K
def item_vectors(model, *, graph=None, item_features=None) -> torch.Tensor:
    """The L2-normalised item rows (native.l2_normalize_rows) of the model's own embedding space, one row per item position, as
    ``diversify_top_k`` and ``intra_list_diversity`` take them.  BasicNCF / MF: the item table the ranking routes build (content
    attached: the item Linear over the content rows).  GraphNCF: the first ``graph.num_items`` rows of ``propagate_all(graph)``.
    AttentionNCF: ItemEmbeddings over the catalogue ``item_features`` — the candidate-side item embedding.  A width over
    ``native.MMR_MAX_D`` is refused (raw content features narrower than that may be passed to ``diversify_top_k`` directly)."""
    _eval_only(model)
    too_wide = "item vectors of {} columns are wider than the {} diversify_top_k takes"
    if _attention_model(model):
        if graph is not None:
            raise ValueError(f"graph= is only taken by a GraphNCF, not by {type(model).__name__}")
        if not torch.is_tensor(item_features) or item_features.dim() != 2:
            raise ValueError("an AttentionNCF embeds a catalogue: pass item_features=(I_c, F) tensor")
        if model.ItemEmbeddings[0].out_features > native.MMR_MAX_D:           # known before any GPU work
            raise ValueError(too_wide.format(model.ItemEmbeddings[0].out_features, native.MMR_MAX_D))
    else:
        if item_features is not None:
            raise ValueError(f"item_features= is only taken by an AttentionNCF, not by {type(model).__name__}")
        if _graph_model(model) and graph is None:
            raise ValueError("a GraphNCF embeds its items on a graph: pass graph=")
        if not _graph_model(model) and graph is not None:
            raise ValueError(f"graph= is only taken by a GraphNCF, not by {type(model).__name__}")
    with torch.no_grad():
        if _attention_model(model):
            require_gpu(item_features)
            rows = model.precompute_catalog(item_features)[0]
        elif graph is not None:
            graph = graph.to(_model_device(model))
            rows = model.propagate_all(graph)[:graph.num_items]
        else:
            rows = model._table("item", model.item_embeddings[0])
        if rows.shape[1] > native.MMR_MAX_D:
            raise ValueError(too_wide.format(rows.shape[1], native.MMR_MAX_D))
        return native.l2_normalize_rows(rows.float())


def diversify_top_k(scores: torch.Tensor, positions: torch.Tensor, counts: Optional[torch.Tensor], item_vectors: torch.Tensor, k: int,
                    lam: float = 0.5, normalize: Optional[str] = "minmax"):
    """Greedy Maximal Marginal Relevance over the candidate pools ``top_k_items`` / ``content_cosine_top_k`` return: from each user's
    pool of N = ``scores.shape[1]`` candidates, ``k`` are picked one after the other, each the candidate with the largest
    ``lam * relevance - (1 - lam) * (largest similarity to a candidate already picked)`` (ncf_mmr_rerank, THE CONTRACT in
    include/ncf_abi.h; one launch for all users).

    scores (B, N) fp32, positions (B, N) int64, counts (B,) int32 or None (every slot in use): a pool per user, on the GPU; it need not
    be sorted, and a slot with position -1 or a non-finite score is never picked.  item_vectors (n_items, D) fp32: row p is the
    vector of item position p, the similarity of two items is the dot product of their rows — pass ``item_vectors(model)`` (unit rows:
    cosines) or raw content features.  lam in [0, 1]: 1 is pure relevance, 0 pure diversity after the first pick.  normalize:
    ``"minmax"`` rescales each pool's scores to [0, 1] over its live slots, so that ``lam`` means the same for every model's score
    range; ``None`` takes the scores as they are.  Limits: N <= 256, D <= 256 and a multiple of 4, k <= min(N, 128).
    Returns ``(scores (B, k) fp32, positions (B, k) int64, counts (B,) int32, mmr (B, k) fp32)`` on the device: the picks in picking
    order with the model scores they had in the pool, and the MMR value each had when picked; slots past ``counts`` hold score -inf,
    position -1 and value -inf.  Every refusal comes before any GPU work; nothing synchronises with the host (a position outside
    ``item_vectors`` is skipped and raises at the next ``native.check_oob``)."""
    if normalize not in (None, "minmax"):
        raise ValueError(f"normalize = {normalize!r} is neither 'minmax' nor None")
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError(f"k = {k!r} is not an int")
    if not isinstance(lam, (int, float)) or isinstance(lam, bool) or not 0.0 <= float(lam) <= 1.0:
        raise ValueError(f"lam = {lam!r} is outside [0, 1]")
    for t, what, dt, dim in ((scores, "scores", torch.float32, 2), (positions, "positions", torch.int64, 2),
                             (item_vectors, "item_vectors", torch.float32, 2)) + (() if counts is None else ((counts, "counts", torch.int32, 1),)):
        if not torch.is_tensor(t) or t.dtype != dt or t.dim() != dim:
            raise ValueError(f"{what} must be a {dim}-D {dt} tensor")
    if positions.shape != scores.shape or (counts is not None and counts.numel() != scores.shape[0]):
        raise ValueError(f"scores is {tuple(scores.shape)}, positions {tuple(positions.shape)}" +
                         ("" if counts is None else f", counts {tuple(counts.shape)}"))
    N, D = scores.shape[1], item_vectors.shape[1]
    if not 1 <= N <= native.MMR_MAX_N:
        raise ValueError(f"a pool of N = {N} candidates is outside 1 .. {native.MMR_MAX_N}")
    if not 4 <= D <= native.MMR_MAX_D or D % 4:
        raise ValueError(f"item vectors of D = {D} columns: D must be a multiple of 4 in 4 .. {native.MMR_MAX_D}")
    if not 1 <= int(k) <= min(N, native.MMR_MAX_K):
        raise ValueError(f"k = {k} is outside 1 .. min(N = {N}, {native.MMR_MAX_K})")
    require_gpu(scores, positions, counts, item_vectors)
    with torch.no_grad():
        scores, positions = scores.contiguous(), positions.contiguous()
        vectors = item_vectors if item_vectors.stride(1) == 1 else item_vectors.contiguous()
        slot, value, count = native.mmr_rerank(vectors, scores, positions, None if counts is None else counts.contiguous(), int(k),
                                               float(lam), normalize == "minmax")
        picked = slot >= 0
        at = slot.clamp_min(0).to(torch.int64)
        out_s = torch.where(picked, scores.gather(1, at), torch.full_like(value, float("-inf")))
        out_p = torch.where(picked, positions.gather(1, at), torch.full_like(at, -1))
    return out_s, out_p, count, value


# ---------------------------------------------------------------------------------------- AttentionNCF: why these items
class Explanations(NamedTuple):
    """What explain_items returns, all on the device; E = max_reasons."""
    positions: torch.Tensor      # (B, k, E) int64 catalogue positions of the rated items that explain a winner; -1 in unused slots
    weights: torch.Tensor        # (B, k, E) fp32 attention weights, descending; 0 in unused slots
    ratings: torch.Tensor        # (B, k, E) fp32 the rating stored for that rated item; 0 in unused slots
    counts: torch.Tensor         # (B, k) int32 rated items above the threshold (not capped at E)
    threshold: torch.Tensor      # (B,) fp32 the threshold of each listed user


def explain_items(model, user_ids: torch.Tensor, item_positions: torch.Tensor, profiles, max_reasons: int = 8,
                  explain_factor: float = 1.5, explain_constant: float = 0.025) -> Explanations:
    """Why an AttentionNCF recommends ``item_positions[b, s]`` to user ``user_ids[b]``: per (user, slot) the rated items whose
    attention weight exceeds ``explain_factor / n_rated + explain_constant`` — the reference's ``because`` and ``attention`` columns
    (webapp/backend.py:105-121) for many users at once, read from the shared logit table (``AttentionNCF.explain``,
    native.attn_explain) without a dense (B * k, I_c) weight matrix.

    user_ids: (B,) int64 rows of ``profiles``' ratings on the GPU.  item_positions: (B, k) int64 catalogue positions, typically
    ``top_k_items(...)[1]``; -1 (a slot past that call's ``counts``) gives an empty explanation.  profiles: ``(item_features
    (I_c, F), ratings)`` with the meaning it has in ``top_k_items``.  max_reasons: E, 1 .. 64 reasons kept per winner.
    The threshold of user u is ``explain_factor / max(n_u, 1) + explain_constant`` in fp32 on the device, n_u = the number of
    STORED entries of the user's row.  The reference's ``n_rated`` also counts a rating whose centred value is exactly 0
    (backend.py:88-92); the CSR does not store those, so for such a user this threshold is slightly higher than the reference's.
    Returns ``Explanations(positions (B, k, E) int64, weights, ratings, counts (B, k) int32, threshold (B,) fp32)`` on the device:
    per winner the qualifying rated items in descending weight (ties: the lower catalogue position for a provider-built row),
    ``counts`` not capped at E, unused slots ``(-1, 0, 0)``.  Needs the logit table (4 * I_c^2 bytes <=
    ``AttentionNCF.cross_table_max_bytes``), not a ``user_emb`` width the cross kernel takes.  Nothing synchronises with the host."""
    _eval_only(model)
    if not _attention_model(model):
        raise ValueError(f"explanations come from attention weights: explain_items takes an AttentionNCF, not {type(model).__name__}")
    if profiles is None:
        raise ValueError("an AttentionNCF explains items for users given by their ratings: pass profiles=(item_features, ratings)")
    if not torch.is_tensor(item_positions) or item_positions.dtype != torch.int64 or item_positions.dim() != 2:
        raise ValueError("item_positions must be a (B, k) int64 tensor of catalogue positions")
    if not 1 <= int(max_reasons) <= native.ATTN_EXPLAIN_MAX_REASONS:
        raise ValueError(f"max_reasons = {max_reasons} is outside 1 .. {native.ATTN_EXPLAIN_MAX_REASONS}")
    if torch.is_tensor(user_ids) and user_ids.dim() == 1 and item_positions.shape[0] != user_ids.numel():
        raise ValueError(f"item_positions has {item_positions.shape[0]} rows for {user_ids.numel()} users")
    r = _resolve_attention(model, user_ids, None, None, profiles, None)
    item_features, ratings = r.profiles
    require_gpu(item_positions, ratings.col, ratings.val)
    with torch.no_grad():
        n_rows = ratings.rowptr.numel() - 1
        if n_rows > 0:
            rows = r.users.clamp(0, n_rows - 1)          # an out-of-range user is refused by the kernel (check_oob), not here
            n = ratings.rowptr[rows + 1] - ratings.rowptr[rows]
        else:
            n = torch.zeros_like(r.users)
        thr = (float(explain_factor) / n.clamp_min(1).to(torch.float32) + float(explain_constant)).contiguous()
        pos, w, val, cnt = model.explain(item_features, ratings, r.users, item_positions.contiguous(), thr, int(max_reasons))
        return Explanations(pos.to(torch.int64), w, val, cnt, thr)


# ---------------------------------------------------------------------------------------- AttentionNCF: item-item attention statistics
class AttentionStats(NamedTuple):
    """What attention_statistics returns, on the device: row = candidate position, column = rated position."""
    sum: torch.Tensor            # (I_c, I_c) float64 attention weight collected by (candidate, rated item) over the samples
    count: torch.Tensor          # (I_c, I_c) int64 samples in which that rated item stood in the candidate's softmax


def attention_statistics(model, user_ids: torch.Tensor, item_positions: torch.Tensor, profiles, out: Optional[AttentionStats] = None) -> AttentionStats:
    """The item-item attention statistics of a sample file under an AttentionNCF — the tables the reference's ``eval_model`` keeps
    for its attention heat-map (eval.py:101-108, 137-143): for every sample (user ``user_ids[s]``, candidate ``item_positions[s]``) and
    every rated item j of that user, ``sum[candidate, j] +=`` the attention weight of j towards the candidate and
    ``count[candidate, j] += 1``.  Read from the shared logit table (``AttentionNCF.attention_stats``, native.attn_stats) without a
    dense (S, I_c) weight matrix.

    user_ids, item_positions: (S,) int64 on the GPU — rows of ``profiles``' ratings and catalogue positions.  profiles:
    ``(item_features (I_c, F), ratings)`` with the meaning it has in ``explain_items``; a row of ``ratings`` lists a catalogue
    position once.  out: the ``AttentionStats`` of an earlier call, continued in place (a file fed in consecutive pieces gives the bits
    of one call; equal inputs give equal bits: every cell is summed in sample order, no atomics).  ``count`` is structural: every
    stored rating counts (the reference's ``user_matrix != 0``), also one whose weight underflowed to 0.  Needs the logit table
    (4 * I_c^2 bytes <= ``AttentionNCF.cross_table_max_bytes``).  An out-of-range user or position adds nothing and raises at the
    next ``native.check_oob``.  Nothing synchronises with the host."""
    _eval_only(model)
    if not _attention_model(model):
        raise ValueError(f"attention statistics come from attention weights: attention_statistics takes an AttentionNCF, not {type(model).__name__}")
    if profiles is None:
        raise ValueError("an AttentionNCF collects attention statistics for users given by their ratings: pass profiles=(item_features, ratings)")
    if not torch.is_tensor(item_positions) or item_positions.dtype != torch.int64 or item_positions.dim() != 1:
        raise ValueError("item_positions must be a (S,) int64 tensor of catalogue positions")
    if torch.is_tensor(user_ids) and user_ids.dim() == 1 and item_positions.numel() != user_ids.numel():
        raise ValueError(f"item_positions has {item_positions.numel()} entries for {user_ids.numel()} users")
    if out is not None and not (isinstance(out, tuple) and len(out) == 2):
        raise ValueError("out must be the AttentionStats of an earlier call")
    r = _resolve_attention(model, user_ids, None, None, profiles, None)
    item_features, ratings = r.profiles
    require_gpu(item_positions, ratings.col)
    return AttentionStats(*model.attention_stats(item_features, ratings, r.users, item_positions, None if out is None else tuple(out)))


def attention_stat_ratios(stats, positions):
    """The sub-tables the reference's heat-map shows (plots.py:172-181): ``(sum, count, ratio)`` as float64 / int64 / float64 numpy
    arrays of shape (n, n) for the n listed catalogue ``positions``, rows and columns in the listed order.  ``ratio`` is the
    reference's formula AS WRITTEN, ``sum / np.max(count, 1)``: the vector of per-row maxima broadcasts over the LAST axis, so cell
    (i, j) is divided by the maximum of row j, not of row i.  A zero maximum gives what numpy gives (inf, or nan for 0 / 0)."""
    pos = np.asarray(positions.cpu() if torch.is_tensor(positions) else positions, dtype=np.int64).reshape(-1)
    to_np = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    s = to_np(stats[0])[pos, :][:, pos]
    c = to_np(stats[1])[pos, :][:, pos]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = s / (np.max(c, 1) if pos.size else np.zeros(0, dtype=c.dtype))
    return s, c, ratio


# ---------------------------------------------------------------------------------------- AttentionNCF: one user, one catalogue
_catalogue_cache = {}


def _catalogue(item_features, device):
    """(features (I, F) fp32 on ``device``, pandas Index of item ids).  A DataFrame is converted once and kept by identity (the last
    one per device), so a serving loop passes the same DataFrame and the model sees the same catalogue tensor every request — which
    is what keeps AttentionNCF's candidate projections.  A ``(tensor, ids)`` pair is used as it is."""
    import pandas as pd
    if isinstance(item_features, tuple):
        feats, ids = item_features
        require_gpu(feats)
        ids = pd.Index(np.asarray(ids.cpu() if torch.is_tensor(ids) else ids))
        if feats.dim() != 2 or feats.shape[0] != len(ids):
            raise ValueError("item_features = (tensor (I, F), ids (I,))")
        return feats, ids
    hit = _catalogue_cache.get(device)
    if hit is not None and hit[0] is item_features:
        return hit[1], hit[2]
    feats = torch.from_numpy(np.ascontiguousarray(item_features.values, dtype=np.float32)).to(device)
    _catalogue_cache[device] = (item_features, feats, item_features.index)
    return feats, item_features.index


def recommend_for_user(model, item_features, user_ratings, k=10, ignore_seen=True, explain_factor=1.5, explain_constant=0.025):
    """The reference's ``recommend_for_user`` (webapp/backend.py:78-121) for an AttentionNCF: same arguments, same meaning, same
    returned DataFrame columns ``imdbID, score, because, attention`` — the ``k`` best items by predicted score, each with the rated
    items whose attention weight exceeds ``explain_factor / n_rated + explain_constant`` and those weights.

    item_features: a DataFrame (index = item ids, one feature row per item) as in the reference, or ``(device tensor (I, F), ids)``.
    user_ratings: a Series of ratings indexed by item id; the ratings are centred as ``rating - (mean + 2.5) / 2`` (backend.py:92).

    Order of work: (1) the whole catalogue is scored once WITHOUT attention weights (the fast path; the catalogue tensor is the
    same object request after request, so the model's kept candidate projections are reused); (2) ncf_topk_rows ranks it on the
    device, skipping the rated items when ``ignore_seen`` (no reduced copy of the catalogue is built); (3) the forward runs again
    with ``return_attention_weights=True`` on the k winners only.  A winner's reported ``score`` comes from pass (1) and its
    ``because`` / ``attention`` from pass (2)'s weights: the two passes compute the same function for the same pair, up to fp32
    summation order.  Ranking ties go to the item that comes first in the catalogue (the reference's sort is not stable)."""
    import pandas as pd
    _eval_only(model)
    if not 1 <= int(k) <= native.TOPK_MAX_K:
        raise ValueError(f"k = {k} is outside 1 .. {native.TOPK_MAX_K}")
    dev = _model_device(model)
    feats, ids = _catalogue(item_features, dev)
    I = feats.shape[0]
    rated_ids = np.sort(np.unique(user_ratings.index))                                 # backend.py:88
    rated_pos = ids.get_indexer(rated_ids)
    if (rated_pos < 0).any():
        raise KeyError(f"rated items not in the catalogue: {list(rated_ids[rated_pos < 0])[:5]}")
    n_rated = len(rated_ids)
    centred = (user_ratings.loc[rated_ids].values - ((user_ratings.mean() + 2.5) / 2)).astype(np.float32)   # backend.py:92
    nz = np.nonzero(centred != 0)[0]          # attention_ncf.py:158: an entry that is exactly 0 counts as unrated
    pos_dev = torch.from_numpy(rated_pos.astype(np.int64)).to(dev)
    rated_items = feats.index_select(0, pos_dev)                                        # backend.py:89
    rowptr = torch.tensor([0, len(nz)], dtype=torch.int64, device=dev)
    col = torch.from_numpy(nz.astype(np.int32)).to(dev)
    val = torch.from_numpy(centred[nz]).to(dev)

    def ratings(B):      # one CSR row shared by every candidate: the reference repeats the user's row B times (backend.py:92)
        return SparseRatings(rowptr, col, val, n_rated, pair_row=torch.zeros(B, dtype=torch.int64, device=dev))

    with torch.no_grad():
        scores = model(feats, rated_items, ratings(I)).view(1, I)
        seen = (torch.tensor([0, n_rated], dtype=torch.int64, device=dev), pos_dev.to(torch.int32)) if ignore_seen else None
        top_s, top_i, top_n = native.topk_rows(scores, k, seen)
        winners = top_i[0].to(torch.int64).clamp_min(0)       # slots past the count rerun item 0 and are dropped below
        _, att = model(RowsOf(feats, winners), rated_items, ratings(winners.numel()), return_attention_weights=True)
        n = int(top_n.item())
        top_s, top_i, att = top_s[0, :n].cpu().numpy(), top_i[0, :n].cpu().numpy(), att[:n].cpu().numpy()

    exp_thr = explain_factor * (1 / max(n_rated, 1)) + explain_constant             # backend.py:105
    mask = att > exp_thr
    if ignore_seen:        # the row label the reference's frame carries: the position in the catalogue without the rated items
        label = top_i - np.searchsorted(np.sort(rated_pos), top_i)
    else:
        label = top_i
    return pd.DataFrame(data={
        'imdbID': ids[top_i],
        'score': top_s,
        'because': [rated_ids[m] for m in mask],
        'attention': [att[i, m] for i, m in enumerate(mask)],
    }, index=label)
