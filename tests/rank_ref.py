"""The contract of the exact-rank entry points (ncf_rank_rows / ncf_dot_rank / ncf_mlp_rank) stated in numpy — the oracle their
tests compare against — and the target / exclusion rows those tests share.

rank[t] = #{non-excluded columns c of the row : key(c) > key(target)}, key = map(score) << 32 | ~column with map() the
order-preserving fp32 -> uint32 map that folds -0.0 onto +0.0 and sends every NaN to 0: descending score, equal scores to the
lower column, NaN below every number and by column.  -1 for a target that is excluded or outside [0, cols).
ranked[r] = the number of non-excluded columns of row r."""
import numpy as np
import torch


def key_map(s):
    """topk_common.h's topk_map on a float32 array -> uint64 (the value of the uint32 map)."""
    s = np.ascontiguousarray(s, dtype=np.float32)
    u = s.view(np.uint32).astype(np.uint64)
    u = np.where(u == 0x80000000, 0, u)                                   # -0.0 == +0.0
    m = np.where(u & 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000)
    return np.where(np.isnan(s), 0, m).astype(np.uint64)


def rank_oracle(scores, seen, targets):
    """(rank (n_targets,) int32, ranked (R,) int32) as torch tensors.  scores: (R, C) fp32 (tensor or array); seen: None or a list
    of per-row id lists (duplicates and ids outside [0, C) do nothing); targets: a list of per-row column lists."""
    s = np.asarray(scores.cpu() if torch.is_tensor(scores) else scores, dtype=np.float32)
    R, C = s.shape
    rank, ranked = [], np.zeros(R, dtype=np.int32)
    for r in range(R):
        keep = np.ones(C, dtype=bool)
        if seen is not None:
            ids = np.asarray(seen[r], dtype=np.int64)
            keep[ids[(ids >= 0) & (ids < C)]] = False
        key = (key_map(s[r]) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(C, dtype=np.uint64))
        live = np.sort(key[keep])
        ranked[r] = len(live)
        for t in targets[r]:
            if t < 0 or t >= C or not keep[t]:
                rank.append(-1)
            else:                                                         # keys are unique: the live keys above the target's
                rank.append(len(live) - int(np.searchsorted(live, key[t], side="right")))
    return torch.tensor(rank, dtype=torch.int32), torch.from_numpy(ranked)


def csr(lists, dev):
    rowptr = torch.tensor(np.concatenate([[0], np.cumsum([len(x) for x in lists])]), dtype=torch.int64, device=dev)
    flat = np.concatenate([np.asarray(x, dtype=np.int64) for x in lists]) if len(lists) else np.zeros(0, dtype=np.int64)
    return rowptr, torch.tensor(flat, dtype=torch.int32, device=dev)


def seen_rows(R, C, rng, shift=0):
    """Per-row exclusion lists, one kind per row in turn (as test_dot_topk_exclusion): empty, a third of the columns, everything,
    unsorted with duplicates and ids outside the list."""
    kinds = [lambda: [],
             lambda: list(range(0, C, 3)),
             lambda: list(range(C)),
             lambda: rng.integers(0, C, max(1, C // 4)).tolist() + [-1, C, C + 50]]
    return [kinds[(r + shift) % len(kinds)]() for r in range(R)]


def target_rows(R, C, cap, rng, seen, shift=0, big=True):
    """Per-row target lists, one kind per row in turn: none, one, `cap`, (big: cap + 1 and 3 cap + 5 — the chunked form), duplicates,
    a target that is in the row's exclusion list, -1 and C as targets, a target in the last column."""
    pick = lambda n: rng.integers(0, C, n).tolist()
    kinds = [lambda r: [],
             lambda r: pick(1),
             lambda r: pick(cap)]
    if big:
        kinds += [lambda r: pick(cap + 1), lambda r: pick(3 * cap + 5)]
    if cap >= 2:
        kinds += [lambda r: (pick(1) * 2 + pick(1) + [0])[:cap],
                  lambda r: ([x for x in (seen[r] if seen else []) if 0 <= x < C][:1] + pick(1))[:cap],
                  lambda r: ([-1, C] + pick(1))[:cap]]
    else:
        kinds += [lambda r: [x for x in (seen[r] if seen else []) if 0 <= x < C][:1] or pick(1), lambda r: [-1], lambda r: [C]]
    kinds += [lambda r: [C - 1]]
    return [kinds[(r + shift) % len(kinds)](r) for r in range(R)]
