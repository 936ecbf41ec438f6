"""AttentionNCF's message dropout as ncf_attn_forward_train applies it, restated in numpy / float64 from include/ncf_abi.h on top of
tests/dropout_mask_ref.py (THE MASK), and the helpers the CPU and GPU tests of it share.

For entry e (its GLOBAL position in the per-pair CSR) with raw score raw_e (b1 and the hidden mask included for the MLP modes, the
dot of the given rows for cosine):
    keep_e = keep_mask(msg_seed, e, 1, msg_p)[:, 0]                 element (entry e, feature 0) of THE MASK under the message seed
    s_e    = keep_e ? raw_e * scale32(msg_p) : 0
    s_e == 0  ->  -inf                                              the reference's `attOut[attOut == 0] = -inf` (attention_ncf.py:189)
then the masked row softmax and the rating-weighted sum, as without it.  thr_m = 0: none of this (the plain kernels).
Nothing here imports the package or needs a GPU."""
import numpy as np
import torch

from attn_forms_ref import masked_softmax64
from dropout_mask_ref import keep_mask, mask_factor64, scale32, threshold

ATT_MLP, ATT_LINEAR, ATT_COS, ATT_MLP_SCALED = 0, 1, 2, 3     # include/ncf_abi.h (native.ATT_*)

# The cases of the kernel comparison, shared by the GPU test and the CPU test that shows its bars attainable in fp32 on the SAME inputs
ROWS = (0, 1, 5, 9, 20, 63, 64, 65, 130, 300, 1000)          # entries per pair: the global index differs from the in-row index
SHAPES = [(A, Fdim) for A in (4, 36, 128, 256) for Fdim in (4, 100, 256)]
MSG_PS = (0.1, 0.3, 0.5)


def msg_seed_of(A, msg_p):
    return 777 + A + int(100 * msg_p)


def hidden_and_message(A):
    """((hidden p, hidden seed), msg_seed, msg_p) of the case with both dropouts active (MLP modes)."""
    return (0.3, 4242 + A), 99 + A, 0.3


def entry_keep(msg_seed, n_entries, msg_p):
    """Boolean (n_entries,): which entries of a per-pair CSR the message dropout keeps."""
    return keep_mask(msg_seed, np.arange(n_entries), 1, msg_p)[:, 0]


def message_logits64(raw, msg_seed, msg_p, zero_rule=True):
    """The logits that enter the softmax, float64 and differentiable in ``raw`` (nnz,).  ``zero_rule=False``: only the entries the
    mask drops leave the softmax (what the rule would be without the reference's ``== 0`` test; the tests show it misses the bar)."""
    if threshold(msg_p) == 0:
        return raw
    keep = torch.from_numpy(entry_keep(msg_seed, raw.numel(), msg_p))
    s = torch.where(keep, raw * float(scale32(msg_p)), torch.zeros_like(raw))
    gone = (s == 0) if zero_rule else ~keep
    return torch.where(gone, torch.full_like(s, -float("inf")), s)


def attention_msgdrop64(mode, pc, pr, w1, b1, rowptr, col, val, feat, bias, seed, p, msg_seed, msg_p, zero_rule=True):
    """attention_dropout64 of tests/dropout_mask_ref.py extended by the entry rule and the zero rule, for the MLP modes and cosine:
    float64 and differentiable in pc, pr, w1, feat.  ``p`` = None or 0: no hidden dropout.  An entry whose column is outside the
    catalogue (a target-masked entry: col = -1) has raw score -inf.  Returns (out (B, Fdim), weights (nnz,), u = pc[b] + pr[col])."""
    B, A = pc.shape
    nnz = col.numel()
    b_of = torch.repeat_interleave(torch.arange(B), rowptr[1:] - rowptr[:-1])
    ok = (col >= 0) & (col < pr.shape[0])
    cc = col.long().clamp(0, pr.shape[0] - 1)
    u = pc[b_of] + pr[cc]
    if mode == ATT_COS:
        raw = (pc[b_of] * pr[cc]).sum(1)
    else:
        h = torch.relu(u)
        if p:
            h = h * mask_factor64(seed, np.arange(nnz), A, p)
        raw = h @ w1 + b1
    raw = torch.where(ok, raw, torch.full_like(raw, -float("inf")))
    w = masked_softmax64(message_logits64(raw, msg_seed, msg_p, zero_rule), rowptr)
    out = torch.zeros(B, feat.shape[1], dtype=torch.float64).index_add_(0, b_of, (w * val.double())[:, None] * feat[cc])
    return out + (0 if bias is None else bias), w, u


def reference(case, seed, p, msg_seed, msg_p, zero_rule=True, dtype=torch.float64):
    """Forward and autograd gradients of a case of _att_case's layout.  ``dtype=torch.float32``: the same torch ops in fp32 (what the
    attainability test holds to the GPU bars); the mask factors are exact in either."""
    leaves = {k: case[k].to(dtype).requires_grad_(True) for k in ("pc", "pr", "w1", "feat")}
    if dtype == torch.float64:
        out, w, u = attention_msgdrop64(case["mode"], leaves["pc"], leaves["pr"], leaves["w1"], case["b1"], case["rowptr"], case["col"],
                                        case["val"], leaves["feat"], case["bias"].double(), seed, p, msg_seed, msg_p, zero_rule)
    else:
        out, w, u = _attention_msgdrop32(case, leaves, seed, p, msg_seed, msg_p)
    grads = torch.autograd.grad(out, [leaves[k] for k in ("pc", "pr", "w1", "feat")], case["dout"].to(dtype), allow_unused=True)
    grads = [torch.zeros_like(leaves[k]) if g is None else g for k, g in zip(("pc", "pr", "w1", "feat"), grads)]
    return out.detach(), w.detach(), dict(zip(("d_pc", "d_pr", "d_w1", "d_feat"), grads)), u.detach()


def _attention_msgdrop32(case, leaves, seed, p, msg_seed, msg_p):
    """The same function in fp32 torch ops (softmax by torch over each row), for the attainability test."""
    pc, pr, w1, feat = (leaves[k] for k in ("pc", "pr", "w1", "feat"))
    rowptr, col, val = case["rowptr"], case["col"], case["val"]
    B, A = pc.shape
    nnz = col.numel()
    b_of = torch.repeat_interleave(torch.arange(B), rowptr[1:] - rowptr[:-1])
    u = pc[b_of] + pr[col.long()]
    if case["mode"] == ATT_COS:
        raw = (pc[b_of] * pr[col.long()]).sum(1)
    else:
        h = torch.relu(u)
        if p:
            h = h * mask_factor64(seed, np.arange(nnz), A, p).float()
        raw = h @ w1 + case["b1"]
    keep = torch.from_numpy(entry_keep(msg_seed, nnz, msg_p))
    s = torch.where(keep, raw * torch.tensor(scale32(msg_p)), torch.zeros_like(raw))
    s = torch.where(s == 0, torch.full_like(s, -float("inf")), s)
    rows = []
    rp = rowptr.tolist()
    for r in range(B):
        x = s[rp[r]:rp[r + 1]]
        rows.append(torch.softmax(x, 0).nan_to_num(0.0) if x.numel() and bool(torch.isfinite(x).any()) else torch.zeros_like(x))
    w = torch.cat(rows)
    out = torch.zeros(B, feat.shape[1]).index_add_(0, b_of, (w * val)[:, None] * feat[col.long()])
    return out + case["bias"], w, u


class EntryMaskDropout:
    """Stands in for torch.nn.functional.dropout in the torch branch of AttentionNCF._forward_train: the 1-D logit vector (one element
    per (pair, rated entry), row-major — the order of the per-pair CSR) is multiplied by the restated entry mask.  Any other call goes to
    the real function."""

    def __init__(self, real, msg_seed, msg_p):
        self.real, self.msg_seed, self.msg_p, self.calls = real, msg_seed, msg_p, 0

    def __call__(self, x, p=0.5, training=True, inplace=False):
        if x.dim() != 1:
            return self.real(x, p, training, inplace)
        assert p == self.msg_p and training
        self.calls += 1
        f = entry_keep(self.msg_seed, x.numel(), p).astype(np.float64) * float(scale32(p))
        return x * torch.from_numpy(f).to(x.dtype)
