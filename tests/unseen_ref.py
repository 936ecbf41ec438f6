"""The contract of ncf_sample_unseen (include/ncf_abi.h) in numpy, written without the kernel's searches: a draw is made by building
the complement explicitly (np.setdiff1d) and popping the r-th element.  Slow and obviously right; the tests compare bits."""
import numpy as np

M32 = 0xFFFFFFFF


def lowbias32(x):
    """The header's mix on uint32 values carried in uint64 arrays (or Python ints)."""
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & M32
    x ^= x >> np.uint64(16)
    return x


def hashes(seed, slots, K):
    """h[b, j] (uint64 holding a uint32) for the int slots ``slots`` (any non-negative values below 2^63) and j = 0 .. K - 1."""
    s = np.asarray(slots, dtype=np.uint64)
    lo, hi = s & np.uint64(M32), s >> np.uint64(32)
    x = lowbias32(((lo * np.uint64(0x9E3779B1)) & M32) ^ np.uint64(int(seed) & M32))
    x = lowbias32(x ^ ((hi * np.uint64(0x85EBCA77)) & M32) ^ np.uint64(0x68E31DA4))
    j1 = (np.arange(1, K + 1, dtype=np.uint64) * np.uint64(0xC2B2AE35)) & M32
    return lowbias32(x[:, None] ^ j1[None, :])


def ranks(seed, slots, K, M):
    """r[b, j] = (h[b, j] * (M - j)) >> 32, in [0, M - j); M >= K."""
    left = np.uint64(M) - np.arange(K, dtype=np.uint64)
    return ((hashes(seed, slots, K) * left[None, :]) >> np.uint64(32)).astype(np.int64)


def unrank(n_items, taken, r):
    """The r-th smallest (0-based) element of [0, n_items) without the sorted distinct ``taken``, without building the complement:
    walk the gaps between taken items.  draw_ref does not use it; test_unseen_cpu checks it against the explicit complement."""
    prev = -1
    for t in list(taken) + [n_items]:
        gap = int(t) - prev - 1
        if r < gap:
            return prev + 1 + r
        r -= gap
        prev = int(t)
    raise IndexError("r is not below the size of the complement")


def draw_ref(seen_rowptr, seen_col, n_items, pick, K, seed, slot0=0):
    """(n, K) int64: the draw of the contract for every pick, by explicit complement and pop.  A pick outside the users or a user with
    fewer than K unseen items gets a row of -1."""
    seen_rowptr, seen_col, pick = np.asarray(seen_rowptr), np.asarray(seen_col), np.asarray(pick)
    users = len(seen_rowptr) - 1
    out = np.full((len(pick), K), -1, dtype=np.int64)
    for b, u in enumerate(pick):
        if not 0 <= u < users:
            continue
        A = seen_col[seen_rowptr[u]:seen_rowptr[u + 1]]
        M = n_items - len(A)
        if K > M:
            continue
        r = ranks(seed, [slot0 + b], K, M)[0]
        if n_items <= 1 << 20:
            left = list(np.setdiff1d(np.arange(n_items, dtype=np.int64), A))
            for j in range(K):
                out[b, j] = left.pop(int(r[j]))
        else:       # a catalogue too large to list: the same pop, by gaps over what is taken so far
            taken = sorted(int(v) for v in A)
            for j in range(K):
                v = unrank(n_items, taken, int(r[j]))
                out[b, j] = v
                taken = sorted(taken + [v])
    return out
