"""numpy restatement of the EASE kernels (csrc/ease.hip; THE CONTRACT of ncf_ease_* in include/ncf_abi.h): Gram rows, weights, scores
and predictions as explicit fp32 operations in the stated orders (numpy's elementwise loops round every product, sum and quotient on
their own), the float64 closed form (np.linalg.inv), an fp32 restatement of the BLOCKED inversion as the device runs it (the same
panel width, the same scalar Gauss-Jordan of the diagonal block, one fp32 ``@`` per panel product) — a yardstick for rounding
growth, not a bit-exact oracle: BLAS and an MFMA k-chain sum in different orders — and the seeded cases the CPU and the GPU tests
share."""
import functools
import os
import re

import numpy as np

from knn_ref import csr_from_rows, transpose_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB = int(re.search(r"#define\s+NCF_EASE_BLOCK\s+(\d+)", open(os.path.join(ROOT, "include", "ncf_abi.h")).read()).group(1))

# (U, I, mean, seed, lambda, binary): the four cases of the issue
CASES = ((400, 96, 12, 1, 5.0, True), (1500, 257, 20, 2, 20.0, True), (3000, 600, 30, 3, 50.0, False), (6000, 1000, 40, 4, 500.0, False))


@functools.lru_cache(maxsize=None)
def case(U, I, mean, seed, lam=None, binary=True):
    """(rowptr int64, col int32, val fp32): item popularity p_i ~ (i + 1)^-0.8, each user holds max(1, floor(Exp(mean))) distinct
    items (at most I) drawn with those weights, values 1.0 or integers 1 .. 5.  ``lam`` only names the case."""
    rng = np.random.default_rng(seed)
    p = (np.arange(I) + 1.0) ** -0.8
    p /= p.sum()
    rows = []
    for _ in range(U):
        n = min(I, max(1, int(np.floor(rng.exponential(mean)))))
        cols = np.sort(rng.choice(I, n, replace=False, p=p))
        vals = np.ones(n, np.float32) if binary else rng.integers(1, 6, n).astype(np.float32)
        rows.append((cols, vals))
    return csr_from_rows(rows)


def gram_ref(rowptr, col, val, num_items):
    """(I, I) fp32: row i walks the users of column i in ascending order; a user's entries are distinct items, so one vectorised update
    per user is the contract's loop over them."""
    colptr, row, tval = transpose_ref(rowptr, col, val, num_items)
    G = np.zeros((num_items, num_items), np.float32)
    for i in range(num_items):
        g = G[i]
        for p in range(colptr[i], colptr[i + 1]):
            e = slice(rowptr[row[p]], rowptr[row[p] + 1])
            g[col[e]] = g[col[e]] + tval[p] * val[e]
    return G


def dense64(rowptr, col, val, num_items):
    X = np.zeros((len(rowptr) - 1, num_items))
    X[np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr)), col] = val
    return X


def inverse64(G, lam):
    return np.linalg.inv(G.astype(np.float64) + float(np.float32(lam)) * np.eye(len(G)))


def weights_ref(P):
    """W[i][j] = -(P[i][j] / P[j][j]), +0.0 on the diagonal, in P's dtype."""
    W = -(P / np.diag(P)[None, :])
    np.fill_diagonal(W, 0.0)
    return W.astype(P.dtype)


def scores_ref(rowptr, col, val, users, W, item_range=None):
    """(B, i1 - i0) fp32: s = +0.0; for the row's entries in stored order: s = s + val_e * W[col_e][j].  A user outside the CSR and a
    column outside the items add nothing."""
    i0, i1 = (0, W.shape[0]) if item_range is None else item_range
    out = np.zeros((len(users), i1 - i0), np.float32)
    for b, u in enumerate(users):
        if not 0 <= u < len(rowptr) - 1:
            continue
        for e in range(rowptr[u], rowptr[u + 1]):
            if 0 <= col[e] < W.shape[0]:
                out[b] = out[b] + np.float32(val[e]) * W[col[e], i0:i1]
    return out


def predict_ref(rowptr, col, val, users, items, W):
    return np.array([scores_ref(rowptr, col, val, [u], W, (i, i + 1))[0, 0] for u, i in zip(users, items)], np.float32)


def diag_inverse_ref(a):
    """The scalar Gauss-Jordan of the diagonal block, in fp32, step by step as ease_diag_kernel does it; None for a bad pivot."""
    a = a.astype(np.float32).copy()
    n = len(a)
    for k in range(n):
        p = a[k, k]
        if not (p > 0 and np.isfinite(p)):
            return None
        rowk = a[k] / p
        rowk[k] = np.float32(1.0) / p
        colk = a[:, k].copy()
        new = a - colk[:, None] * rowk[None, :]
        new[:, k] = -(colk * rowk[k])
        new[k] = rowk
        a = new
    return a


def blocked_inverse_ref(G, lam, nb=None):
    """(G + lam 1)^-1 in fp32 by the blocked right-looking Gauss-Jordan elimination of ncf_ease_invert; zeros for a bad pivot."""
    nb = NB if nb is None else nb
    A = G.astype(np.float32).copy()
    N = len(A)
    A[np.arange(N), np.arange(N)] += np.float32(lam)
    for k0 in range(0, N, nb):
        K = slice(k0, min(N, k0 + nb))
        bw = K.stop - K.start
        D = diag_inverse_ref(A[K, K])
        if D is None:
            return np.zeros_like(A)
        E = A[K].copy()
        E[:, K] = np.eye(bw, dtype=np.float32)
        R = D @ E
        C = -A[:, K]
        C[K] = np.eye(bw, dtype=np.float32)
        A[K] = 0
        A[:, K] = 0
        A = A + C @ R
    return A


def rel_err(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())


def residual(G, lam, P):
    """max |(G + lam 1) P - 1| in float64."""
    N = len(G)
    return float(np.abs((G.astype(np.float64) + float(np.float32(lam)) * np.eye(N)) @ P.astype(np.float64) - np.eye(N)).max())


def kkt(G, lam, W):
    """max off-diagonal |(G + lam 1) W - G| in float64: zero at the minimiser of the EASE objective."""
    G64 = G.astype(np.float64)
    K = (G64 + float(np.float32(lam)) * np.eye(len(G))) @ W.astype(np.float64) - G64
    np.fill_diagonal(K, 0.0)
    return float(np.abs(K).max())


@functools.lru_cache(maxsize=None)
def solved(c):
    """Everything the tests share for case c of CASES, computed once: the CSR, the fp32 Gram restatement, the float64 inverse and
    weights, the blocked fp32 restatement, and its own figures against float64."""
    U, I, mean, seed, lam, binary = CASES[c]
    csr = case(U, I, mean, seed, lam, binary)
    G = gram_ref(*csr, I)
    P64 = inverse64(G, lam)
    Pb = blocked_inverse_ref(G, lam)
    W64 = weights_ref(P64)
    return dict(csr=csr, I=I, lam=lam, G=G, P64=P64, W64=W64, Pb=Pb, Wb=weights_ref(Pb), err_P=rel_err(Pb, P64),
                err_W=rel_err(weights_ref(Pb), W64), res=residual(G, lam, Pb), kkt=kkt(G, lam, weights_ref(Pb)))


def planted_case():
    """40 users x 24 items in three disjoint blocks of 8: user u belongs to block u % 3 and holds all but one item of it.  Returns
    ((rowptr, col, val), held (40,) int64): EASE must put the held item first among the unrated ones."""
    rows, held = [], []
    for u in range(40):
        members = np.arange(8) + 8 * (u % 3)
        h = members[(u // 3) % 8]
        held.append(h)
        cols = members[members != h]
        rows.append((cols, np.ones(len(cols), np.float32)))
    return csr_from_rows(rows), np.array(held, np.int64)


WIDE_I, WIDE_LAM = 2100, 50.0
WIDE_ROWS = {"empty": 200, "one": 201, "n64": 202, "n65": 203, "long": 204}      # rows of 0, 1, 64, 65 and 2049 entries


@functools.lru_cache(maxsize=None)
def wide_case():
    """I = 2100 (two column tiles of a Gram row, three tiles of a score row), values 1 .. 5: 200 users of the generator, then rows of 0,
    1, 64, 65 and 2049 entries — the last one past the staged-row cap of ncf_ease_scores and past the whole-row walk of the Gram."""
    rowptr, col, val = case(200, WIDE_I, 25, 5, None, False)
    rng = np.random.default_rng(55)
    rows = [(col[rowptr[u]:rowptr[u + 1]], val[rowptr[u]:rowptr[u + 1]]) for u in range(200)]
    for n in (0, 1, 64, 65, 2049):
        cols = np.sort(rng.choice(WIDE_I, n, replace=False))
        rows.append((cols, rng.integers(1, 6, n).astype(np.float32)))
    return csr_from_rows(rows)
