"""numpy restatement of the ItemKNN kernels (csrc/knn.hip; THE CONTRACT of ncf_knn_* in include/ncf_abi.h): squared norms, Gram rows,
similarities, the neighbour table and the scores as explicit fp32 operations in the stated orders (``dt=np.float64`` is the float64
twin), a brute-force dense float64 computation, and the seeded cases the CPU and the GPU tests share.

numpy's elementwise loops round every product, sum, quotient and square root on their own, which is what the contract asks for;
nothing here calls np.dot or a reduction on floats."""
import functools

import numpy as np

# Largest |fp32 restatement - float64 twin| over the similarity matrices of base_case() at every (shrink, min_support) of SIM_PARAMS
# (1.278e-7 = 2.14 * 2^-24 at shrink = 0, on similarities up to 0.771), and over the unweighted full-table scores of score_case()
# (2.047e-6 on scores up to 6.92 in magnitude), as test_knn_cpu.py prints them.  The CPU tests hold the fp32 restatement to 8 x these.
F32_VS_F64_MEASURED = 1.278e-7
SCORE_F32_VS_F64_MEASURED = 2.047e-6

SIM_PARAMS = ((0.0, 1), (10.0, 1), (0.0, 2), (10.0, 2))      # (shrink, min_support)
U, I = 70, 150                                                # three column tiles of 64, the last one partial
LONG_USER, EMPTY_USER, ONE_USER = 0, 5, 6                     # rows of 130 / 0 / 1 entries
UNRATED_ITEM, COMMON_ITEM = 17, 3                             # nobody's item; the item of every user who rated anything


def csr_from_rows(rows, dt=np.float32):
    """rows: a list of (cols ascending, vals) per user -> (rowptr int64, col int32, val fp32)."""
    rowptr = np.zeros(len(rows) + 1, np.int64)
    rowptr[1:] = np.cumsum([len(c) for c, _ in rows])
    col = np.concatenate([np.asarray(c, np.int32) for c, _ in rows] + [np.zeros(0, np.int32)])
    val = np.concatenate([np.asarray(v, dt) for _, v in rows] + [np.zeros(0, dt)])
    return rowptr, col.astype(np.int32), val.astype(dt)


def transpose_ref(rowptr, col, val, num_items):
    """(colptr int64, row int32, tval): the entries stably sorted on their column, so a column lists its users in ascending order."""
    users = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    order = np.argsort(col, kind="stable")
    colptr = np.zeros(num_items + 1, np.int64)
    colptr[1:] = np.cumsum(np.bincount(col, minlength=num_items))
    return colptr, users[order].astype(np.int32), val[order]


def tree64(part):
    """Balanced tree over 64 lane partials in lane order: adjacent pairs first, then pairs of pairs, ..."""
    while part.size > 1:
        part = part[0::2] + part[1::2]
    return part[0]


def item_sq_ref(colptr, tval, dt=np.float32):
    n_items = len(colptr) - 1
    sq = np.zeros(n_items, dt)
    for i in range(n_items):
        v = tval[colptr[i]:colptr[i + 1]].astype(dt)
        part = np.zeros(64, dt)
        for s in range(0, len(v), 64):                       # step s / 64 of every lane: lane l adds entry s + l
            step = v[s:s + 64]
            part[:len(step)] = part[:len(step)] + step * step
        sq[i] = tree64(part)
    return sq


def gram_ref(rowptr, col, val, num_items, dt=np.float32):
    """(dot (I, I) dt, co (I, I) int32): row i walks the users of column i in ascending order; a user's entries are distinct items, so
    one vectorised update per user is the contract's loop over them."""
    colptr, row, tval = transpose_ref(rowptr, col, val, num_items)
    dot = np.zeros((num_items, num_items), dt)
    co = np.zeros((num_items, num_items), np.int32)
    v = val.astype(dt)
    for i in range(num_items):
        for p in range(colptr[i], colptr[i + 1]):
            u, w = row[p], dt(tval[p])
            e = slice(rowptr[u], rowptr[u + 1])
            dot[i, col[e]] = dot[i, col[e]] + w * v[e]
            co[i, col[e]] += 1
    return dot, co


def sim_from_gram(dot, co, sq, shrink, min_support):
    """The similarity rule, elementwise in the dtype of ``dot``."""
    dt = dot.dtype.type
    r = np.sqrt(sq.astype(dt))
    n = r[:, None] * r[None, :]
    cf = co.astype(dt)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (dot / n) * (cf / (cf + dt(np.float32(shrink))))
    dead = np.eye(len(sq), dtype=bool) | (co < min_support) | (n == 0) | ~(s > 0)
    return np.where(dead, dt(0), s).astype(dot.dtype)


def sim_ref(rowptr, col, val, num_items, shrink, min_support, dt=np.float32):
    colptr, _, tval = transpose_ref(rowptr, col, val, num_items)
    dot, co = gram_ref(rowptr, col, val, num_items, dt)
    return sim_from_gram(dot, co, item_sq_ref(colptr, tval, dt), shrink, min_support)


def sim_dense64(rowptr, col, val, num_items, shrink, min_support):
    """Brute force: the dense (U, I) float64 matrix, X^T X by matmul, and the rule on it."""
    n_users = len(rowptr) - 1
    X, M = np.zeros((n_users, num_items)), np.zeros((n_users, num_items))
    users = np.repeat(np.arange(n_users), np.diff(rowptr))
    X[users, col], M[users, col] = val.astype(np.float64), 1.0
    dot, co, sq = X.T @ X, (M.T @ M).astype(np.int32), (X * X).sum(0)
    return sim_from_gram(dot, co, sq, shrink, min_support)


def table_ref(S, N):
    """(nb_pos (I, N) int32, nb_sim (I, N), nb_cnt (I,) int32): the N largest positive entries of each row, ties to the lower column."""
    n_items = S.shape[0]
    pos = np.full((n_items, N), -1, np.int32)
    sim = np.zeros((n_items, N), S.dtype)
    cnt = np.zeros(n_items, np.int32)
    for i in range(n_items):
        order = np.argsort(-S[i], kind="stable")
        order = order[S[i, order] > 0][:N]
        cnt[i] = len(order)
        pos[i, :len(order)], sim[i, :len(order)] = order, S[i, order]
    return pos, sim, cnt


def scores_ref(rowptr, col, val, users, table, weighted, fill, dt=np.float32):
    """(B, I) scores of the listed rows by the score rule, slot by slot."""
    pos, sim, cnt = table
    n_items = pos.shape[0]
    out = np.zeros((len(users), n_items), dt)
    for b, u in enumerate(users):
        e = slice(rowptr[u], rowptr[u + 1])
        held = dict(zip(col[e].tolist(), val[e].astype(dt)))
        for i in range(n_items):
            num, den = dt(0), dt(0)
            for t in range(cnt[i]):
                v = held.get(int(pos[i, t]))
                if v is not None:
                    s = dt(sim[i, t])
                    num = num + s * v
                    den = den + s
            out[b, i] = num if not weighted else (num / den if den > 0 else dt(np.float32(fill)))
    return out


# ---------------------------------------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def base_case():
    """The fitted ratings: U = 70, I = 150, centred fp32 values.  Item 17 is nobody's; item 3 is rated by every user with a row; user 0
    holds 130 items (a lane takes three steps of a whole-row walk), user 5 none, user 6 one.  Sparse enough that many pairs are
    co-rated once only (min_support = 2 removes them) and signed, so that some cosines are negative."""
    rng = np.random.default_rng(20260101)
    rows = []
    for u in range(U):
        if u == EMPTY_USER:
            cols = np.zeros(0, np.int64)
        elif u == ONE_USER:
            cols = np.array([COMMON_ITEM])
        else:
            pool = np.setdiff1d(np.arange(I), [UNRATED_ITEM, COMMON_ITEM])
            n = 129 if u == LONG_USER else int(rng.integers(4, 24))
            cols = np.sort(np.concatenate([rng.choice(pool, n, replace=False), [COMMON_ITEM]]))
        rows.append((cols, rng.normal(0.0, 1.0, len(cols)).astype(np.float32)))
    return csr_from_rows(rows)


@functools.lru_cache(maxsize=None)
def base_gram(dt=np.float32):
    rowptr, col, val = base_case()
    colptr, _, tval = transpose_ref(rowptr, col, val, I)
    return gram_ref(rowptr, col, val, I, dt) + (item_sq_ref(colptr, tval, dt),)


@functools.lru_cache(maxsize=None)
def base_sim(shrink, min_support, dt=np.float32):
    dot, co, sq = base_gram(dt)
    return sim_from_gram(dot, co, sq, shrink, min_support)


@functools.lru_cache(maxsize=None)
def base_table(N, shrink, min_support):
    return table_ref(base_sim(shrink, min_support), N)


@functools.lru_cache(maxsize=None)
def integer_case():
    """U = 40, I = 70 (two tiles at col_tile = 64), values in {-2, -1, 1, 2}.  Items 2k and 2k + 1 (k < 10) are rated by the same users
    with the same values, and so are 60 .. 63 and 64 .. 67 across the tile border: every other item sees them at exactly equal
    similarities, which only the lower-position-first rule orders."""
    rng = np.random.default_rng(7)
    X = np.zeros((40, 70), np.float32)
    held = rng.random((40, 70)) < 0.3
    X[held] = rng.choice(np.array([-2, -1, 1, 2], np.float32), int(held.sum()))
    for k in range(10):
        X[:, 2 * k + 1] = X[:, 2 * k]
    for j in (61, 62, 63):
        X[:, j] = X[:, 60]
    for j in (65, 66, 67):
        X[:, j] = X[:, 64]
    return csr_from_rows([(np.flatnonzero(r), r[np.flatnonzero(r)]) for r in X])


@functools.lru_cache(maxsize=None)
def score_case():
    """A ratings CSR other than the fitted one, over the same 150 items: new users.  Row 0: 130 entries (longer than a stage_cap of 64),
    row 1: empty, row 2: one entry, row 3: only the item nobody rated in the fit (no neighbour of any item: den = 0 everywhere),
    rows 4 .. 7: 10 .. 64 entries (64 = exactly a stage_cap of 64)."""
    rng = np.random.default_rng(99)
    rows = []
    for n in (130, 0, 1, -1, 10, 33, 63, 64):
        cols = np.array([UNRATED_ITEM]) if n < 0 else np.sort(rng.choice(I, n, replace=False))
        rows.append((cols, rng.normal(0.0, 1.5, len(cols)).astype(np.float32)))
    return csr_from_rows(rows)


@functools.lru_cache(maxsize=None)
def base_scores(N, shrink, min_support, weighted, fill, fitted=False):
    rowptr, col, val = base_case() if fitted else score_case()
    return scores_ref(rowptr, col, val, np.arange(len(rowptr) - 1), base_table(N, shrink, min_support), weighted, fill)


@functools.lru_cache(maxsize=None)
def cluster_case():
    """I = 50 items in 5 disjoint clusters of 1, 1, 10, 20 and 18 items; each of 60 users rates inside one cluster only."""
    rng = np.random.default_rng(3)
    sizes = (1, 1, 10, 20, 18)
    cluster = np.repeat(np.arange(5), sizes)
    rng.shuffle(cluster)
    rows = []
    for u in range(60):
        members = np.flatnonzero(cluster == u % 5)
        cols = np.sort(rng.choice(members, min(len(members), int(rng.integers(2, 9))), replace=False))
        rows.append((cols, rng.uniform(0.5, 5.0, len(cols)).astype(np.float32)))
    return csr_from_rows(rows), cluster


def ranked_ref(scores, k, item_ids=None, exclude=None):
    """top_k_items' tuple from reference scores by a numpy sort: columns = item_ids (default all), ``exclude`` a list of column sets
    per user; ties to the lower column.  Also returns each user's full order (for ranks)."""
    B = scores.shape[0]
    cols = np.arange(scores.shape[1]) if item_ids is None else np.asarray(item_ids)
    out_s = np.full((B, k), -np.inf, np.float32)
    out_p = np.full((B, k), -1, np.int64)
    cnt = np.zeros(B, np.int32)
    orders = []
    for b in range(B):
        s = scores[b, cols]
        order = np.argsort(-s, kind="stable")
        if exclude is not None:
            order = order[~np.isin(order, list(exclude[b]))]
        orders.append(order)
        top = order[:k]
        cnt[b] = len(top)
        out_s[b, :len(top)], out_p[b, :len(top)] = s[top], cols[top]
    return out_s, out_p, cnt, orders
