"""Case lists and plain restatements for the fp32 MLP scorers (csrc/mlp_fused.hip, mlp_partial.hip) on every form they take.  No
GPU needed: everything here is numpy / torch on the CPU.  The root reference of the family is the kernel-order C oracle
(oracle/ncf_oracle_c.c through oracle/c_oracle.py); tests/test_fused_forms_cpu.py holds that oracle to float64, and
tests/test_gpu_fused_forms.py holds the kernels to the oracle bit for bit.

THE LAUNCH PLAN.  ``fused_plan`` restates launch_inst of mlp_fused.hip: with tiles = ceil(B / 32) and round = 4 x CUs tiles,
  tiles < SMALL_TILES                                  -> the 4-waves-per-tile kernel ("small"), whole batch;
  ids given, 0 < rem = tiles % round, rem * 1000 < round * PERMILLE
                                                       -> full rounds on the one-wave-per-tile kernel ("main", none when
                                                          tiles < round), the ragged rest on "small";
  otherwise (identity ids, rem == 0, or rem at / above the permille share)      -> "main", whole batch.
``ids given`` is idxA and (idxB or EA == K0): a NULL id array cannot be offset, so identity ids never split.  The ABI has no plan
entry for this kernel, so the GPU tests cannot ask which kernel ran: they place batches on both sides of every boundary of this
restatement (``boundaries``) and require the oracle's bits at each.

THE BLOB.  ``pack_blob`` restates ncf_mlp_pack: Wp[q][nt][lane][j] = W[32 nt + (lane & 31)][8 q + 4 (lane >> 5) + j], then b1,
(Wp2, b2), wl, bl, padded to 4 floats (``blob_layout`` of mlp_fused.h).

THE INTEGER CONDITION.  ``int_case`` draws tables, weights and biases as small integers stored in fp32.  When the largest
sum_k |w_k x_k| + |b| of every layer over the batch (``int_margin``, float64) is below 2^24 every partial sum of every chain is an
integer below 2^24, hence exact in fp32 whatever the order: the float64 result is the expected output bit for bit, and the folded
form (PA = TA W1a^T + b1, PB = TB W1b^T, both exact) equals the fused one.  The worst-case bound (9 K0 + 3 per layer-1 neuron,
then 2 N1 times that, ...) passes 2^24 at 256-256-128, so the ranges are narrow (tables, W1 and biases in [-3, 3], W2 and wl in
[-2, 2]) and the condition is asserted on the data, per case.

THE PREFETCH-RING SPLITS.  Layer 1's row ring requests chunk q + XD - 1 while step q computes and switches from table A to table
B at qa = EA / 8.  ``split_list(K0)`` holds the EA at which the switch meets the ring at each position: qa = 1, 2, 3 (the switch
inside the prologue's XD - 1 requests), qa >= 4, and Q1 - qa = 3, 2, 1 (the last requests of the loop), 0 (single table).
"""
import numpy as np
import torch

SMALL_TILES = 768          # NCF_SMALL_TILES
PERMILLE = 850             # NCF_HYBRID_MAX_PERMILLE
XD = 4                     # NCF_X_DEPTH, NCF_FOLD_XD
PART_PERMILLE = 500        # NCF_PART_HYBRID_MAX_PERMILLE

# NCF_FUSED_INSTANCES (K0, N1, N2) and the folded kernels (N1, N2)
INSTANCES = [(64, 256, 128), (64, 256, 0), (64, 128, 0), (64, 128, 64),
             (128, 256, 128), (128, 256, 0), (128, 128, 0), (128, 128, 64),
             (256, 256, 128), (256, 256, 0), (256, 128, 0)]
FOLDED_INSTANCES = [(256, 128), (128, 64), (256, 64), (128, 128)]
HEADLINE = (128, 256, 128)


def dims_of(inst):
    K0, N1, N2 = inst
    return [K0, N1] + ([N2] if N2 else []) + [1]


# ------------------------------------------------------------------------------------------------ the launch plan
def fused_plan(B, cus, ids_ok):
    """[(kernel, pairs), ...] in launch order, as launch_inst of mlp_fused.hip decides it."""
    tiles = (B + 31) // 32
    if tiles < SMALL_TILES:
        return [("small", B)]
    rnd = 4 * cus
    full, rem = divmod(tiles, rnd)
    if ids_ok and rem > 0 and rem * 1000 < rnd * PERMILLE:
        split = full * rnd * 32
        return ([("main", split)] if full else []) + [("small", B - split)]
    return [("main", B)]


def boundaries(cus):
    """The tile counts the plan turns on, for this CU count: ``round``; ``rem_small`` the largest ragged rest that goes to the small
    kernel and ``rem_main = rem_small + 1`` the smallest that costs a full round; ``main_min`` the smallest tile count a batch WITH
    ids runs whole on the main kernel."""
    rnd = 4 * cus
    rem_small = max(r for r in range(1, rnd) if r * 1000 < rnd * PERMILLE)
    main_min = next(t for t in range(SMALL_TILES, SMALL_TILES + 2 * rnd + 1) if fused_plan(32 * t, cus, True) == [("main", 32 * t)])
    return {"round": rnd, "rem_small": rem_small, "rem_main": rem_small + 1, "main_min": main_min}


# ------------------------------------------------------------------------------------------------ the packed blob
def blob_layout(dims):
    """Offsets (floats) of Wp1, b1, (Wp2, b2), wl, bl and the total, as blob_layout of mlp_fused.h."""
    K0, N1 = dims[0], dims[1]
    L, off = {}, 0
    L["wp1"], off = off, off + N1 * K0
    L["b1"], off = off, off + N1
    last = N1
    if len(dims) == 4:
        N2 = dims[2]
        L["wp2"], off = off, off + N2 * N1
        L["b2"], off = off, off + N2
        last = N2
    L["wl"], off = off, off + last
    L["bl"], off = off, off + 4
    L["total"] = off
    return L


def pack_weight(W):
    """Wp[q][nt][lane][j] = W[32 nt + (lane & 31)][8 q + 4 (lane >> 5) + j], flattened."""
    W = np.asarray(W, dtype=np.float32)
    N, K = W.shape
    out = np.empty((K // 8, N // 32, 64, 4), dtype=np.float32)
    for q in range(K // 8):
        for nt in range(N // 32):
            for lane in range(64):
                k = 8 * q + 4 * (lane >> 5)
                out[q, nt, lane] = W[32 * nt + (lane & 31), k:k + 4]
    return out.reshape(-1)


def pack_blob(weights, biases):
    """The blob ncf_mlp_pack writes for fp32 weights [out][in] and biases (None: zeros; ``biases`` None: all zeros)."""
    ws = [np.asarray(w, dtype=np.float32) for w in weights]
    dims = [ws[0].shape[1]] + [w.shape[0] for w in ws]
    bs = [None] * len(ws) if biases is None else list(biases)
    L = blob_layout(dims)
    blob = np.zeros(L["total"], dtype=np.float32)

    def put(off, v, n):
        blob[off:off + n] = 0.0 if v is None else np.asarray(v, dtype=np.float32).reshape(-1)

    blob[L["wp1"]:L["wp1"] + ws[0].size] = pack_weight(ws[0])
    put(L["b1"], bs[0], dims[1])
    if len(ws) == 3:
        blob[L["wp2"]:L["wp2"] + ws[1].size] = pack_weight(ws[1])
        put(L["b2"], bs[1], dims[2])
    put(L["wl"], ws[-1], ws[-1].size)
    put(L["bl"], bs[-1], 1)
    return blob


# ------------------------------------------------------------------------------------------------ the table splits
def split_list(K0):
    """EA values (EB = K0 - EA) at which the A -> B table switch meets layer 1's row ring at every position."""
    if K0 == 64:
        return list(range(8, 65, 8))
    return sorted({8, 16, 24, K0 // 2, K0 - 24, K0 - 16, K0 - 8, K0})


# ------------------------------------------------------------------------------------------------ data
def random_mlp(g, dims, scale=1.0):
    ws = [torch.randn(dims[i + 1], dims[i], generator=g) * (scale / dims[i] ** 0.5) for i in range(len(dims) - 1)]
    bs = [torch.randn(dims[i + 1], generator=g) * 0.1 for i in range(len(dims) - 1)]
    return ws, bs


def _ints(g, shape, r):
    return torch.randint(-r, r + 1, shape, generator=g).to(torch.float32)


def int_case(g, EA, EB, hidden, rowsA, rowsB):
    """Tables, weights and biases of small integers in fp32 (see THE INTEGER CONDITION)."""
    dims = [EA + EB] + list(hidden) + [1]
    ta, tb = _ints(g, (rowsA, EA), 3), (_ints(g, (rowsB, EB), 3) if EB else None)
    ws = [_ints(g, (dims[i + 1], dims[i]), 3 if i == 0 else 2) for i in range(len(dims) - 1)]
    bs = [_ints(g, (dims[i + 1],), 3) for i in range(len(dims) - 1)]
    return ta, tb, ws, bs


def _gather64(tab, idx, B):
    """Rows of ``tab`` in float64 under the kernels' range rule, finite tables only: an out-of-range row reads as zeros."""
    i = torch.arange(B) if idx is None else idx.long()
    ok = (i >= 0) & (i < tab.shape[0])
    return tab.double()[torch.where(ok, i, torch.zeros_like(i))] * ok.double().unsqueeze(1)


def score_f64(tabA, tabB, idxA, idxB, weights, biases, B=None, margins=None):
    """The table-form forward in float64 (cat -> Linear, ReLU ... -> 1-wide Linear), out-of-range rows as zeros.  ``margins``
    (a list) receives max over the batch and the neurons of sum_k |w_k x_k| + |b| per layer."""
    if B is None:
        B = len(idxA) if idxA is not None else (len(idxB) if idxB is not None else tabA.shape[0])
    x = _gather64(tabA, idxA, B)
    if tabB is not None:
        x = torch.cat((x, _gather64(tabB, idxB, B)), 1)
    for i, (w, b) in enumerate(zip(weights, biases)):
        b64 = torch.zeros(w.shape[0], dtype=torch.float64) if b is None else b.double()
        if margins is not None:
            margins.append(float((x.abs() @ w.double().abs().t() + b64.abs()).max()) if B else 0.0)
        x = x @ w.double().t() + b64
        if i + 1 < len(weights):
            x = torch.relu(x)
    return x


def int_margin(tabA, tabB, idxA, idxB, weights, biases, B=None):
    """Largest sum |w x| + |b| of any layer over the batch: below 2^24 every fp32 partial sum on integer data is exact."""
    m = []
    score_f64(tabA, tabB, idxA, idxB, weights, biases, B, margins=m)
    return max(m)


def fold_tables(ta, tb, W1, b1):
    """(PA, PB) of the folded form in float64 -> fp32: PA = TA W1[:, :EA]^T + b1, PB = TB W1[:, EA:]^T (exact on integer data)."""
    EA = ta.shape[1]
    PA = ta.double() @ W1[:, :EA].double().t() + b1.double()
    PB = tb.double() @ W1[:, EA:].double().t()
    return PA.float(), PB.float()


# ------------------------------------------------------------------------------------------------ the one comparison
def assert_same_bits(got, ref, what=""):
    """NaN at the same positions (a NaN's payload differs between host and device), int32-view equality everywhere else."""
    got, ref = got.detach().cpu().reshape(-1), ref.detach().cpu().reshape(-1)
    assert got.dtype == torch.float32 and ref.dtype == torch.float32 and got.shape == ref.shape, what
    gn, rn = torch.isnan(got), torch.isnan(ref)
    assert torch.equal(gn, rn), f"{what}: NaN at other positions ({int(gn.sum())} vs {int(rn.sum())})"
    bad = (got.view(torch.int32) != ref.view(torch.int32)) & ~rn
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} differ, first at {i}: {got[i].item()!r} vs {ref[i].item()!r}")
