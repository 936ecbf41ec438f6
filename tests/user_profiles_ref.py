"""The contract of ncf_user_profiles (include/ncf_abi.h, csrc/user_profiles.hip) restated as a plain float64 loop, the vectorised numpy
expression it equals, and the cases the CPU and GPU tests share.

    acc = 0.0 (double)
    for e in row u, in order:
        acc = acc + ((double)rating[e] - avg[u]) * (double)features[col[e], f]      (product rounded, then sum rounded)
    out[u, f] = (float)(acc / (double)n_u)

An empty row gives zeros; an entry whose column is outside [0, I) adds nothing (n_u still counts it).
"""
import numpy as np

F_LIST = (1, 3, 4, 64, 67, 256, 260, 300)
ROW_LENGTHS = (0, 1, 2, 7, 8, 9, 63, 64, 65, 700)
N_ITEMS = 900
N_USERS = 37


def profiles_loop(rowptr, col, rating, avg, features):
    """The contract, one entry at a time; every operation is one IEEE double operation per column (numpy elementwise: no fused
    multiply-add, no reordering).  Returns (U, F) float32."""
    feat = np.asarray(features)
    U, (I, F) = len(avg), feat.shape
    out = np.zeros((U, F), dtype=np.float32)
    for u in range(U):
        beg, end = int(rowptr[u]), int(rowptr[u + 1])
        if end == beg:
            continue
        acc = np.zeros(F, dtype=np.float64)
        for e in range(beg, end):
            c = int(col[e])
            if not 0 <= c < I:
                continue
            d = np.float64(rating[e]) - np.float64(avg[u])
            acc = acc + d * feat[c].astype(np.float64)
        out[u] = (acc / np.float64(end - beg)).astype(np.float32)
    return out


def profiles_numpy(rowptr, col, rating, avg, features):
    """The reference's expression per user (create_user_embedding): ((r - avg).reshape(-1, 1) * feat[col]).mean(axis=0) in float64,
    rounded to fp32; zeros for a user without ratings.  Columns must be in range."""
    feat = np.asarray(features).astype(np.float64)
    U = len(avg)
    out = np.zeros((U, feat.shape[1]), dtype=np.float32)
    for u in range(U):
        beg, end = int(rowptr[u]), int(rowptr[u + 1])
        if end > beg:
            r = np.asarray(rating[beg:end]).astype(np.float64)
            out[u] = ((r - avg[u]).reshape(-1, 1) * feat[np.asarray(col[beg:end])]).mean(axis=0).astype(np.float32)
    return out


def make_case(F, lengths, seed, n_items=N_ITEMS):
    """One CSR of len(lengths) users: ascending distinct columns per row, half-star ratings (0.5 .. 5.0), an arbitrary float64 avg per
    user and normal fp32 features.  Returns a dict of numpy arrays."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    rowptr = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=rowptr[1:])
    col = np.concatenate([np.sort(rng.choice(n_items, int(n), replace=False)) for n in lengths] + [np.zeros(0, np.int64)]).astype(np.int32)
    rating = (rng.integers(1, 11, int(rowptr[-1])) * 0.5).astype(np.float32)
    avg = rng.uniform(1.5, 3.75, len(lengths)) + rng.standard_normal(len(lengths)) * 1e-3
    features = rng.standard_normal((n_items, F)).astype(np.float32)
    return {"rowptr": rowptr, "col": col, "rating": rating, "avg": avg.astype(np.float64), "features": features}


def user_lengths(n_users=N_USERS, seed=0):
    """Row lengths of the many-user case: every length of ROW_LENGTHS at least three times, in a shuffled order."""
    reps = -(-n_users // len(ROW_LENGTHS))
    lengths = np.tile(np.asarray(ROW_LENGTHS), reps)[:n_users]
    return np.random.default_rng(seed).permutation(lengths)


def cases(F):
    """(name, case) over the issue's list for one width: U = 37 with every row length, and U = 1 with each row length."""
    yield f"F{F}-U{N_USERS}", make_case(F, user_lengths(), seed=1000 + F)
    for n in ROW_LENGTHS:
        yield f"F{F}-U1-n{n}", make_case(F, [n], seed=2000 + 7 * F + n)
