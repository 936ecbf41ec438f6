"""The in-kernel dropout mask of ncf_spmm_csr_dropout / ncf_attn_forward_dropout / ncf_attn_backward, restated in numpy from
include/ncf_abi.h ("THE MASK"), and the float64 references the GPU tests hold those kernels to.

The mask is a pure function of (seed, entry e modulo 2^32, 16-byte chunk c = features 4c .. 4c+3):
    h0 = lowbias32(e * 0x9E3779B1 ^ seed ^ c * 0x85EBCA77),  h1 = lowbias32(h0 ^ 0x68E31DA4)            (uint32 arithmetic)
    features 4c, 4c+1, 4c+2, 4c+3 are kept iff h0 & 0xFFFF, h0 >> 16, h1 & 0xFFFF, h1 >> 16 are >= thr
    thr = (uint32)(p * 65536.f + 0.5f) in fp32, clamped to 65535;  kept values times the fp32 quotient 65536.f / (float)(65536 - thr)
Nothing here imports the package or needs a GPU."""
import numpy as np
import torch


def lowbias32(x):
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def threshold(p):
    """thr of the header: the fp32 arithmetic of the library (halves round UP, unlike Python's round), clamped to 65535."""
    t = np.float32(p) * np.float32(65536.0) + np.float32(0.5)
    assert t.dtype == np.float32
    return min(int(t), 65535)                      # the C cast truncates; t >= 0.5 here


def scale32(p):
    """What kept values are multiplied by: 1 / (1 - p') rounded to fp32, as an np.float32.  Exactly 1 for thr = 0."""
    s = np.float32(65536.0) / np.float32(65536 - threshold(p))
    assert s.dtype == np.float32
    return s


def p_quantised(p):
    return threshold(p) / 65536.0


def keep_mask(seed, entries, n_features, p):
    """Boolean (len(entries), n_features): True where element (entry, feature) is kept.  ``entries`` are taken modulo 2^32."""
    e = (np.asarray(entries, dtype=np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    chunks = (int(n_features) + 3) // 4
    c = np.arange(chunks, dtype=np.uint32)
    thr = np.uint32(threshold(p))
    with np.errstate(over="ignore"):
        h0 = lowbias32((e[:, None] * np.uint32(0x9E3779B1)) ^ np.uint32(int(seed) & 0xFFFFFFFF) ^ (c[None, :] * np.uint32(0x85EBCA77)))
        h1 = lowbias32(h0 ^ np.uint32(0x68E31DA4))
    keep = np.stack([(h0 & np.uint32(0xFFFF)) >= thr, (h0 >> np.uint32(16)) >= thr,
                     (h1 & np.uint32(0xFFFF)) >= thr, (h1 >> np.uint32(16)) >= thr], axis=2)
    return keep.reshape(e.shape[0], 4 * chunks)[:, :n_features]


def mask_factor64(seed, entries, n_features, p):
    """float64 torch tensor (len(entries), n_features): scale (the fp32 value widened) where kept, 0 where dropped."""
    return torch.from_numpy(keep_mask(seed, entries, n_features, p).astype(np.float64) * float(scale32(p)))


# ------------------------------------------------------------------------------------------------ float64 references
def spmm_dropout64(rowptr, col, coef, z, n_rows, ids, seed, p):
    """y[r] = sum over the CSR entries k of row r of coef_k * scale * keep(seed, ids[k], f) * z[col_k], in float64 by index_add_.
    Also returns sum_k |term| per output element: the scale of the summation-order error of a long row."""
    nnz = col.numel()
    D = z.shape[1]
    row = torch.repeat_interleave(torch.arange(n_rows), rowptr[1:] - rowptr[:-1])
    w = torch.ones(nnz, dtype=torch.float64) if coef is None else coef.double()
    terms = w[:, None] * mask_factor64(seed, ids.numpy() if ids is not None else np.arange(nnz), D, p) * z.double()[col.long()]
    y = torch.zeros(n_rows, D, dtype=torch.float64).index_add_(0, row, terms)
    mag = torch.zeros(n_rows, D, dtype=torch.float64).index_add_(0, row, terms.abs())
    return y, mag


def attention_dropout64(pc, pr, w1, b1, rowptr, col, val, feat, bias, seed, p, softmax):
    """The attention of ncf_attn_forward_dropout on a per-pair CSR, float64 and differentiable in pc, pr, w1, feat:
    s_e = b1 + sum_a w1[a] relu(pc[b,a] + pr[col_e,a]) * scale * keep(seed, e, a) with e the entry's GLOBAL position; ``softmax`` is
    masked_softmax64 of tests/test_gpu_attention_softmax.py.  Returns (out (B, Fdim), weights (nnz,), u = pc[b] + pr[col] (nnz, A))."""
    B, A = pc.shape
    nnz = col.numel()
    b_of = torch.repeat_interleave(torch.arange(B), rowptr[1:] - rowptr[:-1])
    u = pc[b_of] + pr[col.long()]
    h = torch.relu(u) * mask_factor64(seed, np.arange(nnz), A, p)
    s = h @ w1 + b1
    w = softmax(s, rowptr)
    out = torch.zeros(B, feat.shape[1], dtype=torch.float64).index_add_(0, b_of, (w * val.double())[:, None] * feat[col.long()])
    return out + (0 if bias is None else bias), w, u
