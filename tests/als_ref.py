"""numpy restatement of the ImplicitALS kernels (csrc/als.hip; THE CONTRACT of ncf_als_gram / ncf_als_solve_rows in include/ncf_abi.h):
the chunked Gram matrix (``gram_ref``), one half-sweep over listed rows with its segments, Cholesky, substitutions and flag bits
(``solve_rows_ref``), whole fits (``fit_ref``), the float64 objective, a dense closed form through ``np.linalg.solve`` and the seeded
cases the CPU and the GPU tests share.  ``dt=np.float64`` turns every fp32 loop into its float64 twin.

numpy's elementwise operations round every product, sum, difference, quotient and square root on their own, which is what the
contract asks for.  The elimination and the substitutions are written right-looking (a column is finished, then subtracted from
everything after it): every element still has its products subtracted one by one in ascending k (descending, for the backward
substitution), which is the order the contract fixes."""
import functools

import numpy as np

from knn_ref import transpose_ref          # numpy's stable argsort on the column: the transpose ItemKNN and ImplicitALS both fit on

MAX_FACTORS, GRAM_ROWS, SEG = 128, 256, 512
FLAG_COL, FLAG_PTR, FLAG_ORDER, FLAG_VAL, FLAG_PIVOT = 1, 2, 4, 8, 16
F_LIST = (1, 3, 32, 33, 64, 100, 128)       # one tile; a ragged tile edge at R = 1; whole tiles at R = 2, 4, 8; ragged ones at R = 4, 8
U, I, NNZ = 37, 23, 250
REG, ALPHA = 0.1, 4.0
SENTINEL = 7.25                             # what the padding columns of a device table hold
LONG_I = 1100
LONG_LENS = (1050, 0, 1, 64, 65, 512)       # three segments, the last ragged; empty; one entry; around a staging step; exactly one segment
GRAM_ROWS_LIST = (1, 255, 256, 257, 600)

# Largest |fp32 half-sweep - float64 twin| of the user half-sweep of the base case over F_LIST (test_als_cpu.py prints it per F):
# 3.7e-7 at F = 1 up to 5.472e-5 at F = 128, on solutions whose entries reach 3.7 (the normal matrices have condition numbers near
# 1e3: reg = 0.1 under eigenvalues of tens).  The CPU test holds the fp32 restatement to 8 x this, on one half-sweep only: whole fits
# are compared bit for bit and never by tolerance.  The float64 twin is within 9.5e-14 of the dense closed form.
F32_VS_F64_MEASURED = 5.472e-5


def gram_ref(T, F, dt=np.float32):
    """G = T^T T over the first F columns of T, by chunks of 256 rows."""
    T = np.asarray(T)[:, :F].astype(dt)
    G = np.zeros((F, F), dt)
    for r0 in range(0, T.shape[0], GRAM_ROWS):
        P = np.zeros((F, F), dt)
        for t in T[r0:r0 + GRAM_ROWS]:
            P = P + np.outer(t, t)
        G = G + P
    G = np.tril(G)
    return G + np.tril(G, -1).T


def cholesky_solve_ref(A, b):
    """x = A^-1 b by the contract's Cholesky and substitutions, in A's dtype; None when a pivot is not > 0 or not finite."""
    A, c = np.tril(A).copy(), b.copy()
    F = A.shape[0]
    for j in range(F):
        s = A[j, j]
        if not (s > 0 and np.isfinite(s)):
            return None
        d = np.sqrt(s)
        A[j, j] = d
        A[j + 1:, j] = A[j + 1:, j] / d
        A[j + 1:, j + 1:] = A[j + 1:, j + 1:] - np.outer(A[j + 1:, j], A[j + 1:, j])
    for k in range(F):
        c[k] = c[k] / A[k, k]
        c[k + 1:] = c[k + 1:] - A[k + 1:, k] * c[k]
    for k in range(F - 1, -1, -1):
        c[k] = c[k] / A[k, k]
        c[:k] = c[:k] - A[k, :k] * c[k]
    return c


def solve_rows_ref(rowptr, col, val, rows, T, G, alpha, reg, F, dt=np.float32, out=None, out_by_row=False):
    """One half-sweep of the listed rows; returns ``(out, flag bits)``.  ``out`` (default: zeros of (len(rows), F), or of
    (len(rowptr) - 1, F) with ``out_by_row``) keeps every row the sweep does not write."""
    rowptr, col, rows = np.asarray(rowptr, np.int64), np.asarray(col), np.asarray(rows, np.int64)
    R, nnz, n_t = len(rowptr) - 1, len(col), T.shape[0]
    Tm, Gm, vals = np.asarray(T)[:, :F].astype(dt), np.asarray(G).astype(dt), np.asarray(val)
    alpha, reg, one = dt(np.float32(alpha)), dt(np.float32(reg)), dt(1)
    if out is None:
        out = np.zeros((R if out_by_row else len(rows), F), dt)
    flag = 0
    for k, row in enumerate(rows):
        if not 0 <= row < R:
            flag |= FLAG_PTR
            if not out_by_row:
                out[k] = 0
            continue
        o = row if out_by_row else k
        beg, end = int(rowptr[row]), int(rowptr[row + 1])
        out[o] = 0
        if beg < 0 or end > nnz or end < beg:
            flag |= FLAG_PTR
            continue
        if end == beg:
            continue
        bad = False
        A, b = Gm.copy(), np.zeros(F, dt)
        for s0 in range(beg, end, SEG):
            S = np.zeros((F, F), dt)
            for e in range(s0, min(end, s0 + SEG)):
                c, v = int(col[e]), vals[e]
                okc, okv = 0 <= c < n_t, bool(v >= 0 and v < np.inf)
                flag |= (0 if okc else FLAG_COL) | (0 if okv else FLAG_VAL)
                if e > beg and col[e - 1] >= col[e]:
                    flag |= FLAG_ORDER
                    bad = True
                if not (okc and okv):
                    continue
                t, w = Tm[c], alpha * dt(v)
                S = S + np.outer(w * t, t)
                b = b + (one + w) * t
            A = A + S
        A[np.arange(F), np.arange(F)] = A[np.arange(F), np.arange(F)] + reg
        x = cholesky_solve_ref(A, b)
        if x is None:
            flag |= FLAG_PIVOT
            bad = True
        if not bad:
            out[o] = x
    return out, flag


def solve_rows_dense64(rowptr, col, val, rows, T, alpha, reg, F):
    """The closed form in float64: (T^T T + T_u^T diag(alpha v) T_u + reg I)^-1 T_u^T (1 + alpha v), through np.linalg.solve."""
    T64 = np.asarray(T)[:, :F].astype(np.float64)
    G = T64.T @ T64
    out = np.zeros((len(rows), F))
    for k, row in enumerate(rows):
        beg, end = int(rowptr[row]), int(rowptr[row + 1])
        if end == beg:
            continue
        Tu, w = T64[col[beg:end]], float(np.float32(alpha)) * val[beg:end].astype(np.float64)
        A = G + Tu.T @ (w[:, None] * Tu) + float(np.float32(reg)) * np.eye(F)
        out[k] = np.linalg.solve(A, Tu.T @ (1.0 + w))
    return out


def objective64(rowptr, col, val, X, Y, alpha, reg):
    """sum over the entries of c (1 - s)^2 - s^2, + sum_u x_u^T (Y^T Y) x_u, + reg (|X|^2 + |Y|^2), in float64: the iALS objective
    (every unobserved pair has confidence 1 and preference 0)."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    us = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    s = (X[us] * Y[col]).sum(1)
    c = 1.0 + float(np.float32(alpha)) * np.asarray(val, np.float64)
    return float((c * (1.0 - s) ** 2 - s * s).sum() + ((X @ (Y.T @ Y)) * X).sum() + float(np.float32(reg)) * ((X * X).sum() + (Y * Y).sum()))


def fit_ref(rowptr, col, val, num_items, X0, Y0, n_iters, reg, alpha, dt=np.float32, loss=False):
    """``n_iters`` iterations (the user half-sweep, then the item half-sweep over the transposed CSR) from the tables X0 / Y0; returns
    ``(X, Y, losses)``, the float64 objective after every half-sweep when ``loss`` is set."""
    F = X0.shape[1]
    X, Y = X0.astype(dt), Y0.astype(dt)
    colptr, trow, tval = transpose_ref(rowptr, col, val, num_items)
    users, items = np.arange(len(rowptr) - 1), np.arange(num_items)
    losses = []
    for _ in range(n_iters):
        X, f1 = solve_rows_ref(rowptr, col, val, users, Y, gram_ref(Y, F, dt), alpha, reg, F, dt)
        if loss:
            losses.append(objective64(rowptr, col, val, X, Y, alpha, reg))
        Y, f2 = solve_rows_ref(colptr, trow, tval, items, X, gram_ref(X, F, dt), alpha, reg, F, dt)
        if loss:
            losses.append(objective64(rowptr, col, val, X, Y, alpha, reg))
        assert f1 == 0 and f2 == 0
    return X, Y, losses


# ---------------------------------------------------------------------------------------- the shared cases
@functools.lru_cache(maxsize=None)
def base_case():
    """(rowptr, col, val): U = 37 users over I = 23 items, 250 distinct entries, the last user and the last item empty, values
    multiples of 0.5 in 0.5 .. 5."""
    rng = np.random.default_rng(20240)
    cells = rng.choice((U - 1) * (I - 1), NNZ, replace=False)
    cells.sort()
    us, it = cells // (I - 1), (cells % (I - 1)).astype(np.int32)
    rowptr = np.zeros(U + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(us, minlength=U))
    val = (rng.integers(1, 11, NNZ) * 0.5).astype(np.float32)
    for a in (rowptr, it, val):
        a.setflags(write=False)
    return rowptr, it, val


@functools.lru_cache(maxsize=None)
def table(rows, F, seed, ld=None, sd=0.3):
    """A (rows, ld) fp32 table: N(0, sd) factors in the first F columns, SENTINEL in the padding."""
    ld = F if ld is None else ld
    t = np.full((rows, ld), SENTINEL, np.float32)
    t[:, :F] = (np.random.default_rng(seed).standard_normal((rows, F)) * sd).astype(np.float32)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def base_gram(F, dt=np.float32):
    return gram_ref(table(I, F, 100 + F), F, dt)


@functools.lru_cache(maxsize=None)
def base_sweep(F, dt=np.float32):
    """The user half-sweep of the base case against table(I, F, 100 + F): ((U, F) rows, flag bits)."""
    rowptr, col, val = base_case()
    return solve_rows_ref(rowptr, col, val, np.arange(U), table(I, F, 100 + F), base_gram(F, dt), ALPHA, REG, F, dt)


@functools.lru_cache(maxsize=None)
def long_case():
    """(rowptr, col, val) of rows of LONG_LENS entries over LONG_I items."""
    rng = np.random.default_rng(77)
    cols = [np.sort(rng.choice(LONG_I, n, replace=False)).astype(np.int32) for n in LONG_LENS]
    rowptr = np.zeros(len(LONG_LENS) + 1, np.int64)
    rowptr[1:] = np.cumsum(LONG_LENS)
    col = np.concatenate(cols)
    val = (rng.integers(0, 11, len(col)) * 0.5).astype(np.float32)          # zeros too: an entry of confidence 1
    for a in (rowptr, col, val):
        a.setflags(write=False)
    return rowptr, col, val


@functools.lru_cache(maxsize=None)
def long_sweep(F):
    rowptr, col, val = long_case()
    T = table(LONG_I, F, 300 + F, ld=F + 3, sd=0.1)
    return solve_rows_ref(rowptr, col, val, np.arange(len(LONG_LENS)), T, gram_ref(T, F), ALPHA, REG, F)


@functools.lru_cache(maxsize=None)
def gram_case(rows, F):
    T = table(rows, F, 500 + rows + F, ld=F + 5)
    return T, gram_ref(T, F)


FIT_F, FIT_ITERS, FIT_SEED, FIT_SD = 8, 3, 11, 0.1


def initial_tables(num_users, num_items, F, sd, seed, rowptr, col):
    """ImplicitALS.fit's draws from a CPU generator seeded with ``seed``: one normal_ of (U, F), then one of (I, F); rows without any
    entry are zero."""
    import torch
    g = torch.Generator().manual_seed(seed)
    X = torch.empty((num_users, F), dtype=torch.float32).normal_(0.0, sd, generator=g).numpy()
    Y = torch.empty((num_items, F), dtype=torch.float32).normal_(0.0, sd, generator=g).numpy()
    X[np.diff(rowptr) == 0] = 0
    Y[np.bincount(col, minlength=num_items) == 0] = 0
    return X, Y


@functools.lru_cache(maxsize=None)
def base_fit(dt=np.float32):
    """(X, Y, losses) of FIT_ITERS iterations on the base case at F = FIT_F."""
    rowptr, col, val = base_case()
    X0, Y0 = initial_tables(U, I, FIT_F, FIT_SD, FIT_SEED, rowptr, col)
    return fit_ref(rowptr, col, val, I, X0, Y0, FIT_ITERS, REG, ALPHA, dt, loss=True)


PLANT_G, PLANT_N, PLANT_F, PLANT_ITERS = 4, 6, 8, 10


@functools.lru_cache(maxsize=None)
def planted_case():
    """4 user groups x 4 item groups of 6: user j of group g holds every item of group g but item j of it, which is held out.
    Returns ``((rowptr, col, val), held_out (U,) item positions)``."""
    n = PLANT_G * PLANT_N
    rowptr, col, held = np.zeros(n + 1, np.int64), [], np.zeros(n, np.int64)
    for u in range(n):
        g, j = divmod(u, PLANT_N)
        held[u] = g * PLANT_N + j
        col += [g * PLANT_N + i for i in range(PLANT_N) if i != j]
        rowptr[u + 1] = len(col)
    col = np.asarray(col, np.int32)
    return (rowptr, col, np.ones(len(col), np.float32)), held


@functools.lru_cache(maxsize=None)
def planted_fit():
    (rowptr, col, val), _ = planted_case()
    n = PLANT_G * PLANT_N
    X0, Y0 = initial_tables(n, n, PLANT_F, FIT_SD, FIT_SEED, rowptr, col)
    return fit_ref(rowptr, col, val, n, X0, Y0, PLANT_ITERS, REG, ALPHA)[:2]
