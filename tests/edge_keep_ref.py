"""The edges one GraphNCF training step keeps (ncf_edge_keep, PreparedGraph.batch_coef, GraphNCF._draw_node_keep), restated in numpy
from include/ncf_abi.h ("THE KEEP RULE").  Reference mapping: gnn_ncf.py:246-279 (message dropout), :281-296 (node dropout),
:314-320 (the batch's target edges).

Message dropout:  thr = (uint32)(p * 65536.f + 0.5f) clamped to 65535;  h = lowbias32((uint32)slot * 0x9E3779B1 ^ (uint32)seed);
    kept iff (h >> 16) >= thr.  slot of edge j of user2item is j; of edge j of item2user also j when the two lists have the same
    length and both attributes are present (one mask bit for both directions), else E1 + j.
Node dropout:  every batch node is kept; of the others the K = int((1.0 - p) * (N - nb)) smallest by (key(n), n),
    key(n) = lowbias32((uint32)n * 0x9E3779B1 ^ (uint32)node_seed); an edge survives iff both its ends are kept.
Nothing here imports the package or needs a GPU."""
import numpy as np

from dropout_mask_ref import lowbias32, threshold


def _hash(ids, seed):
    x = (np.asarray(ids, dtype=np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    with np.errstate(over="ignore"):
        return lowbias32((x * np.uint32(0x9E3779B1)) ^ np.uint32(int(seed) & 0xFFFFFFFF))


def message_keep(seed, slots, p):
    """Boolean per slot: True where the edge with that slot is kept."""
    return (_hash(slots, seed) >> np.uint32(16)) >= np.uint32(threshold(p))


def node_keep(node_seed, N, batch_nodes, p):
    """uint8 (N,): 1 for every batch node and for the K other nodes with the smallest (key, n)."""
    in_batch = np.zeros(N, dtype=bool)
    in_batch[np.asarray(batch_nodes, dtype=np.int64)] = True
    nb = int(in_batch.sum())
    K = int((1.0 - p) * (N - nb))
    n = np.arange(N, dtype=np.int64)
    key = _hash(n, node_seed).astype(np.int64)
    others = n[~in_batch]
    others = others[np.lexsort((others, key[others]))]               # by key, ties by node id
    keep = in_batch.copy()
    keep[others[:K]] = True
    return keep.astype(np.uint8)


def symmetric(u2i, i2u, a1, a2):
    return u2i.shape[1] == i2u.shape[1] and a1 is not None and a2 is not None


def slots(u2i, i2u, a1, a2):
    E1, E2 = u2i.shape[1], i2u.shape[1]
    return np.arange(E1, dtype=np.int64), np.arange(E2, dtype=np.int64) + (0 if symmetric(u2i, i2u, a1, a2) else E1)


def keep_lists(u2i, i2u, a1, a2, N, users=None, items=None, p=0.0, seed=0, node_mask=None):
    """Boolean keep per edge of each list (numpy int64 (2, E) lists).  ``users`` / ``items``: the batch whose target edges are
    removed in both directions (None: no target masking); ``node_mask``: uint8 (N,) or None."""
    k1, k2 = np.ones(u2i.shape[1], dtype=bool), np.ones(i2u.shape[1], dtype=bool)
    if users is not None:
        key = np.asarray(users, dtype=np.int64) * N + np.asarray(items, dtype=np.int64)
        k1 &= ~np.isin(u2i[0] * N + u2i[1], key)
        k2 &= ~np.isin(i2u[1] * N + i2u[0], key)
    if node_mask is not None:
        nm = np.asarray(node_mask).astype(bool)
        k1 &= nm[u2i[0]] & nm[u2i[1]]
        k2 &= nm[i2u[0]] & nm[i2u[1]]
    s1, s2 = slots(u2i, i2u, a1, a2)
    k1 &= message_keep(seed, s1, p)
    k2 &= message_keep(seed, s2, p)
    return k1, k2


def edge_keep_ref(u2i, i2u, a1, a2, N, users=None, items=None, p=0.0, seed=0, node_mask=None):
    """(w float32 per CSR entry, deg int32 (N,)): the entry's weight where kept (1 when either attribute is missing), 0 where removed,
    and the number of kept entries per destination.  CSR order = stable argsort by destination of cat(u2i, i2u), as PreparedGraph."""
    k1, k2 = keep_lists(u2i, i2u, a1, a2, N, users, items, p, seed, node_mask)
    dst = np.concatenate([u2i[1], i2u[1]])
    order = np.argsort(dst, kind="stable")
    keep = np.concatenate([k1, k2])
    weight = np.ones(dst.size, dtype=np.float32) if (a1 is None or a2 is None) else np.concatenate([a1, a2]).astype(np.float32)
    w = np.where(keep, weight, np.float32(0.0)).astype(np.float32)[order]
    deg = np.bincount(dst[keep], minlength=N).astype(np.int32)
    return w, deg
