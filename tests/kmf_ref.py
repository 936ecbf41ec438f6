"""numpy restatement of the KernelMF kernels (csrc/kmf.hip; THE CONTRACT of ncf_kmf_epoch in include/ncf_abi.h): the stratified SGD
epoch as an fp32 loop (``epoch_ref``; ``dt=np.float64`` is its float64 twin), the plan builder of ``KernelMF.fit`` restated, the
fold-in (``fold_users_ref``) and the seeded cases the CPU and the GPU tests share.

Tables here are compact: (rows, F + 1), the factors and then the bias.  numpy's elementwise loops round every product and every sum
on their own, which is what the contract asks for."""
import functools

import numpy as np

F_LIST = (1, 3, 4, 64, 65, 100, 255, 256)     # one lane; a ragged last lane; whole lanes; all 64 lanes; the bias in each lane position
W_LIST = (1, 2, 5, 23, 64)                     # 5: no power of two; 23 = I; 64 > U: whole strata are empty
U, I, N = 37, 23, 600
LR, REG = 0.05, 0.02
SENTINEL = 7.25                                # what the padding columns of a device table hold

# Largest |fp32 table - float64 twin table| after 3 epochs over every (F, W) of F_LIST x W_LIST (test_kmf_cpu.py prints it):
# 2.767e-7 = 4.64 * 2^-24 (at F = 65, W = 2) on tables whose entries stay below 0.87.  The CPU test holds the fp32 loop to 8 x this.
F32_VS_F64_MEASURED = 2.767e-7


def sample_step(P, Q, F, u, i, r, mu, lr, reg, item_side=True):
    """One sample of the contract on compact tables, in the tables' dtype; returns err."""
    dt = P.dtype.type
    p, q = P[u, :F].copy(), Q[i, :F].copy()
    bu, bi = P[u, F], Q[i, F]
    t = np.zeros(256, dt)
    t[:F] = p * q
    t = t.reshape(64, 4)                       # column c is lane c // 4; a column past F adds +0.0, which changes no bit of a sum that
    part = np.zeros(64, dt)                    # started from +0.0
    for j in range(4):
        part = part + t[:, j]
    while part.size > 1:                       # adjacent pairs first, then pairs of pairs, ...
        part = part[0::2] + part[1::2]
    pred = ((mu + bi) + bu) + part[0]
    err = pred - r
    P[u, F] = bu - lr * (err + reg * bu)
    P[u, :F] = p - lr * (err * q + reg * p)
    if item_side:
        Q[i, F] = bi - lr * (err + reg * bi)
        Q[i, :F] = q - lr * (err * p + reg * q)
    return err


def epoch_ref(P, Q, F, plan, mu, lr, reg, n_epochs=1, reverse=False, checked=True):
    """``n_epochs`` epochs over ``plan`` (build_plan's dict), in place on P (U, F + 1) and Q (I, F + 1); returns the (n_epochs, W)
    float64 sums of squared errors.  ``reverse``: a stratum's blocks in descending order.  ``checked``: skip what the kernel flags;
    the flag bits come back as the second value of epoch_ref_flags."""
    return epoch_ref_flags(P, Q, F, plan, mu, lr, reg, n_epochs, reverse, checked)[0]


def epoch_ref_flags(P, Q, F, plan, mu, lr, reg, n_epochs=1, reverse=False, checked=True):
    dt = P.dtype.type
    assert Q.dtype == P.dtype and P.shape[1] == Q.shape[1] == F + 1
    mu, lr, reg = dt(np.float32(mu)), dt(np.float32(lr)), dt(np.float32(reg))
    W, ptr, n = plan["W"], plan["block_ptr"], len(plan["user"])
    us, it, rs = plan["user"], plan["item"], plan["rating"].astype(dt)
    ub, ib = plan["user_block"], plan["item_block"]
    sse = np.zeros((n_epochs, W), np.float64)
    flag = 0
    for e in range(n_epochs):
        for s in range(W):
            for a in (range(W - 1, -1, -1) if reverse else range(W)):
                beg, end = int(ptr[s * W + a]), int(ptr[s * W + a + 1])
                if beg < 0 or end > n or end < beg:
                    flag |= 4
                    beg = end = 0
                acc = 0.0
                for k in range(beg, end):
                    u, i = int(us[k]), int(it[k])
                    if checked:
                        if not (0 <= u < P.shape[0] and 0 <= i < Q.shape[0]):
                            flag |= 1
                            continue
                        if ub[u] != a or ib[i] != (a + s) % W:
                            flag |= 2
                            continue
                    err = float(sample_step(P, Q, F, u, i, rs[k], mu, lr, reg))
                    acc = acc + err * err
                sse[e, a] = sse[e, a] + acc
    return sse, flag


def sequential_ref(P, Q, F, user, item, rating, mu, lr, reg):
    """The plain per-sample pass over the input order (what W = 1 must be)."""
    dt = P.dtype.type
    mu, lr, reg = dt(np.float32(mu)), dt(np.float32(lr)), dt(np.float32(reg))
    acc = 0.0
    for u, i, r in zip(user, item, rating.astype(dt)):
        err = float(sample_step(P, Q, F, int(u), int(i), r, mu, lr, reg))
        acc = acc + err * err
    return acc


def fold_users_ref(P, Q, F, users, rowptr, col, rating, mu, lr, reg, n_epochs=1):
    """ncf_kmf_fold_users on compact tables: in place on the listed rows of P, Q only read; returns (sse (n_epochs, n_users), flag)."""
    dt = P.dtype.type
    mu, lr, reg = dt(np.float32(mu)), dt(np.float32(lr)), dt(np.float32(reg))
    rs = rating.astype(dt)
    sse = np.zeros((n_epochs, len(users)), np.float64)
    flag = 0
    for k, u in enumerate(users):
        u = int(u)
        if not 0 <= u < P.shape[0]:
            flag |= 1
            continue
        beg, end = int(rowptr[k]), int(rowptr[k + 1])
        if beg < 0 or end > len(col) or end < beg:
            flag |= 4
            beg = end = 0
        for e in range(n_epochs):
            acc = 0.0
            for j in range(beg, end):
                i = int(col[j])
                if not 0 <= i < Q.shape[0]:
                    flag |= 1
                    continue
                err = float(sample_step(P, Q, F, u, i, rs[j], mu, lr, reg, item_side=False))
                acc = acc + err * err
            sse[e, k] = acc
    return sse, flag


def deal_blocks(ids, count, W):
    """Ids dealt to W blocks round-robin in descending order of their number of ratings; the sort is stable, ties go by position."""
    counts = np.bincount(ids, minlength=count)
    order = np.argsort(-counts, kind="stable")
    block = np.empty(count, np.int32)
    block[order] = (np.arange(count) % W).astype(np.int32)
    return block


def build_plan(user, item, rating, num_users, num_items, W):
    """KernelMF.fit's plan restated: stratum-major blocks, input order kept inside a block."""
    user, item = np.asarray(user, np.int64), np.asarray(item, np.int64)
    ub, ib = deal_blocks(user, num_users, W), deal_blocks(item, num_items, W)
    a, b = ub[user].astype(np.int64), ib[item].astype(np.int64)
    key = ((b - a) % W) * W + a
    order = np.argsort(key, kind="stable")
    ptr = np.zeros(W * W + 1, np.int64)
    np.cumsum(np.bincount(key, minlength=W * W), out=ptr[1:])
    return {"W": W, "user": user[order].astype(np.int32), "item": item[order].astype(np.int32),
            "rating": np.asarray(rating, np.float32)[order], "block_ptr": ptr, "user_block": ub, "item_block": ib, "order": order}


@functools.lru_cache(maxsize=None)
def ratings_case(n=N, seed=0):
    """Rank-4 synthetic ratings in 0.5 .. 5 (multiples of 0.5): (user, item, rating, mu).  The last user and the last item have no
    rating; a run of samples repeats one user and a few (user, item) pairs come twice."""
    rng = np.random.default_rng(seed)
    us, it = rng.integers(0, U - 1, n), rng.integers(0, I - 1, n)
    if n >= 32:
        us[10:14] = us[10]                     # the same user four samples in a row
        us[20:23], it[20:23] = us[5:8], it[5:8]   # duplicate (u, i) samples
    tp, tq = rng.normal(0, 1, (U, 4)), rng.normal(0, 1, (I, 4))
    r = np.clip(np.round((2.75 + 0.6 * (tp[us] * tq[it]).sum(1)) * 2) / 2, 0.5, 5).astype(np.float32)
    mu = np.float32(r.astype(np.float64).mean())
    for a in (us, it, r):
        a.setflags(write=False)
    return us, it, r, mu


def init_tables(F, seed=1, dt=np.float32):
    """Compact start tables: factors N(0, 0.1), small non-zero biases (fp32 values, in ``dt``)."""
    g = np.random.default_rng(seed)
    P = np.concatenate([g.normal(0, .1, (U, F)), g.normal(0, .05, (U, 1))], 1).astype(np.float32)
    Q = np.concatenate([g.normal(0, .1, (I, F)), g.normal(0, .05, (I, 1))], 1).astype(np.float32)
    return P.astype(dt), Q.astype(dt)


@functools.lru_cache(maxsize=None)
def plan_case(W, n=N):
    us, it, r, mu = ratings_case(n)
    return build_plan(us, it, r, U, I, W)


@functools.lru_cache(maxsize=None)
def epoch_case(F, W, n=N, dt=np.float32):
    """The reference of one (F, W) case, computed once: ((P1, Q1, sse1) after 1 epoch, (P3, Q3, sse3) after 3).  Read-only."""
    mu = ratings_case(n)[3]
    plan = plan_case(W, n)
    P, Q = init_tables(F, dt=dt)
    sse = [epoch_ref(P, Q, F, plan, mu, LR, REG)]
    one = (P.copy(), Q.copy(), sse[0].copy())
    sse.append(epoch_ref(P, Q, F, plan, mu, LR, REG, 2))
    three = (P, Q, np.concatenate(sse))
    for t in one + three:
        t.setflags(write=False)
    return one, three


def padded(T, F, ld):
    """A device-shaped table: (rows, ld) with the compact table in columns 0 .. F and SENTINEL beyond."""
    out = np.full((T.shape[0], ld), SENTINEL, np.float32)
    out[:, :F + 1] = T
    return out


def leading_dim(F, pad):
    return (F + 1 + 31) // 32 * 32 if pad else F + 1


def fold_case(F, seed=4):
    """Users 3, 36 (no row yet: U - 1 has no rating), 11 and 0 with 0 .. 70 ratings each (one row empty, one longer than a wave)."""
    g = np.random.default_rng(seed)
    users = np.array([3, U - 1, 11, 0], np.int32)
    lens = np.array([70, 5, 0, 17])
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = g.integers(0, I, int(lens.sum())).astype(np.int32)
    rating = (g.integers(1, 11, int(lens.sum())) * 0.5).astype(np.float32)
    return users, rowptr, col, rating
