"""ctypes binding of oracle/libncf_oracle_c.so (the kernel-order C restatement) — TEST INFRASTRUCTURE ONLY."""
import ctypes
import os
import subprocess

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libncf_oracle_c.so")


def _load():
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < os.path.getmtime(os.path.join(_HERE, "ncf_oracle_c.c")):
        subprocess.check_call(["make", "-s", "-C", _HERE])
    lib = ctypes.CDLL(_LIB)
    p, i64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.oracle_score_fused_f32.restype = ci
    lib.oracle_score_fused_f32.argtypes = [p, i64, p, i64, p, p, i64, ci, ci, p, p, ci, p, p, ci, p, p, p]
    lib.oracle_score_fused_f32_ex.restype = ci
    lib.oracle_score_fused_f32_ex.argtypes = [p, i64, i64, p, i64, i64, p, p, i64, ci, ci, p, p, ci, p, p, ci, p, p, p, p]
    lib.oracle_layer1_partial_f32.restype = ci
    lib.oracle_layer1_partial_f32.argtypes = [p, i64, i64, ci, ci, p, p, ci, p]
    lib.oracle_score_folded_f32.restype = ci
    lib.oracle_score_folded_f32.argtypes = [p, i64, i64, p, i64, i64, p, p, i64, ci, p, p, ci, p, p, p, p]
    return lib


def score_fused_f32(tabA, tabB, idxA, idxB, weights, biases):
    """Same arguments as the table-form forward; weights/biases are the MLP's (W, b) in order, last layer 1 wide."""
    lib = _load()
    c = lambda t: np.ascontiguousarray(t.detach().cpu().numpy())
    ta, tb = c(tabA.float()), c(tabB.float())
    ia, ib = c(idxA.long()), c(idxB.long())
    ws = [c(w.float()) for w in weights]
    bs = [c(b.float()) for b in biases]
    B = ia.shape[0]
    out = np.empty(B, dtype=np.float32)
    two = len(ws) == 3
    W2 = ws[1] if two else np.zeros(1, np.float32)
    b2 = bs[1] if two else np.zeros(1, np.float32)
    rc = lib.oracle_score_fused_f32(ta.ctypes.data, ta.shape[1], tb.ctypes.data, tb.shape[1], ia.ctypes.data, ib.ctypes.data, B,
                                    ta.shape[1], tb.shape[1], ws[0].ctypes.data, bs[0].ctypes.data, ws[0].shape[0],
                                    W2.ctypes.data, b2.ctypes.data, ws[1].shape[0] if two else 0,
                                    ws[-1].ctypes.data, bs[-1].ctypes.data, out.ctypes.data)
    if rc != 0:
        raise ValueError("shape not tileable like the fused kernel")
    return torch.from_numpy(out).view(-1, 1)


# ---------------------------------------------------------------------------------------------------------------------
# The extended oracle: the root reference of the fp32 scorer family.  Tensors live on the CPU; strided tables are taken as they
# are read (their values), ids may be None (identity: pair p reads row p), tabB may be None (single-table form, EB = 0) and any
# bias may be None (zeros).  Every entry returns (scores (B, 1) float32, whether any id was out of range).
def _f32(t):
    return None if t is None else np.ascontiguousarray(t.detach().cpu().to(torch.float32).numpy())


def _i64(t):
    return None if t is None else np.ascontiguousarray(t.detach().cpu().to(torch.int64).numpy())


def _p(a):
    return None if a is None else a.ctypes.data


def _batch(B, ia, ib, rowsA):
    if B is not None:
        return int(B)
    return ia.shape[0] if ia is not None else (ib.shape[0] if ib is not None else rowsA)


def _mlp_arrays(weights, biases):
    ws = [_f32(w) for w in weights]
    bs = [_f32(b) for b in biases]
    if len(ws) not in (2, 3) or ws[-1].shape[0] != 1:
        raise ValueError("the oracle restates one or two hidden layers and a 1-wide last layer")
    two = len(ws) == 3
    return ws, bs, (ws[1] if two else None), (bs[1] if two else None), (ws[1].shape[0] if two else 0)


def score_fused_f32_ex(tabA, tabB, idxA, idxB, weights, biases, B=None):
    """ncf_score_fused restated: the kernels' range rule (row 0 times 0.0f), identity ids, EB = 0 and NULL biases included."""
    lib = _load()
    ta, tb, ia, ib = _f32(tabA), _f32(tabB), _i64(idxA), _i64(idxB)
    ws, bs, W2, b2, N2 = _mlp_arrays(weights, biases)
    EA, EB = ta.shape[1], (tb.shape[1] if tb is not None else 0)
    if ws[0].shape[1] != EA + EB:
        raise ValueError("tables and first layer disagree")
    B = _batch(B, ia, ib, ta.shape[0])
    out = np.empty(B, dtype=np.float32)
    oob = ctypes.c_int(0)
    rc = lib.oracle_score_fused_f32_ex(_p(ta), ta.shape[0], EA, _p(tb), tb.shape[0] if tb is not None else 0, EB, _p(ia), _p(ib), B,
                                       EA, EB, _p(ws[0]), _p(bs[0]), ws[0].shape[0], _p(W2), _p(b2), N2, _p(ws[-1]), _p(bs[-1]),
                                       _p(out), ctypes.addressof(oob))
    if rc != 0:
        raise ValueError("shape not tileable like the fused kernel")
    return torch.from_numpy(out).view(-1, 1), bool(oob.value)


def layer1_partial_f32(tabA, W1, b1):
    """P (rowsA + 1, N1) of ncf_layer1_partial: layer 1's chain from b1 cut after table A's k-groups; the last row is row 0 times 0."""
    lib = _load()
    ta, w, b = _f32(tabA), _f32(W1), _f32(b1)
    P = np.empty((ta.shape[0] + 1, w.shape[0]), dtype=np.float32)
    if lib.oracle_layer1_partial_f32(_p(ta), ta.shape[0], ta.shape[1], ta.shape[1], w.shape[1], _p(w), _p(b), w.shape[0], _p(P)) != 0:
        raise ValueError("shape not tileable like the partial kernel")
    return torch.from_numpy(P)


def score_folded_f32(PA, PB, idxA, idxB, tail_weights, tail_biases, B=None):
    """ncf_score_folded restated: s = PA_row * zA + PB_row * zB, ReLU, then the tail MLP [N1 -> N2 -> 1] in kernel order."""
    lib = _load()
    pa, pb, ia, ib = _f32(PA), _f32(PB), _i64(idxA), _i64(idxB)
    ws, bs = [_f32(w) for w in tail_weights], [_f32(b) for b in tail_biases]
    if len(ws) != 2 or ws[1].shape[0] != 1 or pa.shape[1] != ws[0].shape[1] or pb.shape[1] != pa.shape[1]:
        raise ValueError("folded tables and tail MLP disagree")
    B = _batch(B, ia, ib, pa.shape[0])
    out = np.empty(B, dtype=np.float32)
    oob = ctypes.c_int(0)
    rc = lib.oracle_score_folded_f32(_p(pa), pa.shape[0], pa.shape[1], _p(pb), pb.shape[0], pb.shape[1], _p(ia), _p(ib), B,
                                     pa.shape[1], _p(ws[0]), _p(bs[0]), ws[0].shape[0], _p(ws[1]), _p(bs[1]), _p(out),
                                     ctypes.addressof(oob))
    if rc != 0:
        raise ValueError("shape not tileable like the folded kernel")
    return torch.from_numpy(out).view(-1, 1), bool(oob.value)
