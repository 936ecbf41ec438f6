"""References, inputs and case tables for the attention kernels of csrc/attn.hip (CPU only: nothing here touches a GPU).

Four kernels, each with several launch forms chosen by shape:
  attn_kernel            one wave per pair.  Phase 1 (logits) is VECTOR when A % 4 == 0, A <= 256 and ldpc, ldpr % 4 == 0: LPA = 8, 16,
                         32 or 64 lanes share an entry (A / 4 16-byte chunks, rounded up to a power of two: lanes c >= chunks idle);
                         else GENERIC (a lane per entry).  Phase 3 (aggregation) likewise on Fdim, ldfeat, ldout with LPF; its
                         generic form walks the features in passes of 64.  Blocks are renumbered for XCD locality.
  attn_backward_kernel   the same LPF (phase 1) and LPA (phase 2) lane splits, float atomics into d_pr / d_feat.
  attn_grouped_sc_kernel <MODE in {0, 2, 3}, CPB in {32, 16, 8, 1}, NW in {4, 8}>: tiles of 64 entries staged by LDS-DMA (source-chunk
                         XOR swizzle when A % 64 == 0; a readlane path for rows of 16 / 32 / 64 chunks, a divide path otherwise),
                         aggregation on 16 x 16 MFMA tiles (partial column tile when Fdim % 16 != 0).
  attn_grouped_kernel    <MODE in {0, 2}, FO in {1, 2, 4}, NPF in {4, 8, 16}>: tiles staged through registers.

``per_pair_form`` / ``grouped_form`` mirror the dispatch; the tables below reach every form; ``make_inputs`` builds inputs on which
a wrong index shows: exact logits (so the float64 reference and the kernels see the same softmax arguments), every entry visible in
the softmax (spread <= 8), every operand a column slice of a wider poisoned buffer, outputs pre-filled with a sentinel, masked
entries, an all-masked row, empty rows, hot items.  The checks (``check_forward``, ``check_backward``) are shared by the GPU tests
and by the CPU emulators of tests/test_attn_forms_cpu.py, which show that each of ten index defects fails them."""
import collections
import functools

import numpy as np
import torch

ATT_MLP, ATT_LINEAR, ATT_COS, ATT_MLP_SCALED = 0, 1, 2, 3     # include/ncf_abi.h (native.ATT_*)
SCALE_LOG2 = 64                                               # native.ATT_SCALE_LOG2
B1 = 0.125
POISON = 1024.0            # padding columns of every input
SENTINEL = -777.25         # every output word before the call
SPREAD_MAX = 8.0           # max logit - min logit of a row: exp(-8) = 3.4e-4, every entry carries weight
LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)
N_ITEMS = 300
WTS_PAD = 16               # sentinel words after the weights
MODE_NAMES = {ATT_MLP: "mlp", ATT_LINEAR: "linear", ATT_COS: "cos", ATT_MLP_SCALED: "mlps"}


# ------------------------------------------------------------------------------------------------ float64 reference (CPU)
def masked_softmax64(s, rowptr):
    """Row softmax over the CSR entries ``s`` (float64, -inf = masked); a row without a finite entry gets zeros (the reference's
    F.softmax over -inf + nan_to_num, attention_ncf.py:208-209)."""
    s = s.double()
    w = torch.zeros_like(s)
    rp = rowptr.tolist()
    for r in range(len(rp) - 1):
        x = s[rp[r]:rp[r + 1]]
        if x.numel() and bool(torch.isfinite(x).any()):
            e = torch.exp(x - x.max())
            w[rp[r]:rp[r + 1]] = e / e.sum()
    return w


def scores64(mode, pc, pr, w1, b1, normalize=True):
    """Logits of pairs ``pc`` (P, A) against entries ``pr`` (n, A): (P, n) float64.  MLP / MLP_SCALED: b1 + sum_a w1[a] relu(pc + pr);
    LINEAR (A = 1): pc + pr; COS: dot of the L2-normalised rows (eps 1e-12; ``normalize=False``: the kernels' contract, rows given
    normalised — what the backward differentiates)."""
    if mode == ATT_LINEAR:
        return pc[:, None, 0] + pr[None, :, 0]
    if mode == ATT_COS:
        if normalize:
            pc, pr = torch.nn.functional.normalize(pc, dim=1, eps=1e-12), torch.nn.functional.normalize(pr, dim=1, eps=1e-12)
        return pc @ pr.t()
    return torch.relu(pc[:, None, :] + pr[None]) @ w1 + b1


def attention64(mode, pc, pr, w1, b1, rowptr, col, val, pair_row, feat, bias, normalize=True):
    """out (B, Fdim) = sum_e w_e val_e feat[col_e] + bias per pair (bias alone for an empty set), the weights and the logits in the
    expanded per-pair CSR layout (pair b's entries, pairs in order), all float64 and differentiable in pc, pr, w1, feat."""
    B, I = pc.shape[0], pr.shape[0]
    rp = rowptr.tolist()
    out = [None] * B
    wts, logits = [None] * B, [None] * B
    for r in range(len(rp) - 1):
        pairs = (pair_row == r).nonzero().view(-1)
        if not pairs.numel():
            continue
        c, v = col[rp[r]:rp[r + 1]].long(), val[rp[r]:rp[r + 1]].double()
        ok = (c >= 0) & (c < I)
        cc = c.clamp(0, max(I - 1, 0))
        if c.numel():
            s = scores64(mode, pc[pairs], pr[cc], w1, b1, normalize)
            s = torch.where(ok[None], s, torch.full_like(s, -float("inf")))
            w = torch.softmax(s, 1).nan_to_num(0.0) if bool(ok.any()) else torch.zeros_like(s)
            o = (w * v) @ feat[cc] + bias
        else:
            s = w = torch.zeros((pairs.numel(), 0), dtype=torch.float64)
            o = bias.expand(pairs.numel(), -1) + 0 * feat.sum() + 0 * pc[pairs].sum()
        for k, b in enumerate(pairs.tolist()):
            out[b], wts[b], logits[b] = o[k], w[k], s[k]
    return torch.stack(out), torch.cat(wts), torch.cat(logits)


def backward_bars(mode, pc, pr, w1, col, owner, val_e, feat, dout, w, rtol=1e-5):
    """Per-element bars of the attention backward's d_pc, d_pr and d_w1: ``rtol`` x T plus the fp32 flush floor.

    Entry e (expanded layout; only entries with a valid column are passed) belongs to pair ``owner[e]``, rates item ``col[e]`` with
    ``val_e[e]`` and got the float64 weight ``w[e]``.  The gradients go through the softmax derivative g_e = w_e (dv_e - sum_j w_j
    dv_j), dv_e = val_e feat[col_e] . dout_b, which cancels on a peaked row; T is the float64 sum of the ABSOLUTE values of the terms of
    an element (|g_e| taken as w_e (|dv_e| + sum_j w_j |dv_j|), times |w1[a]| relu'(pc + pr) for d_pc / d_pr, relu(pc + pr) for d_w1,
    the other operand's |row| for COS): an fp32 sum of those terms in any order is within a few ulp of T of the exact value.  The floor
    is the same sum with every g_e replaced by 2^-126 (1 + |dv_e| + sum_j w_j |dv_j|): weights below fp32's normal range flush.
    MLP modes also assert that pc + pr is never 0 (no relu kink: the derivative is defined everywhere)."""
    pcd, prd = pc.double(), pr.double()
    B = pc.shape[0]
    dv = val_e.double() * (feat.double()[col] * dout.double()[owner]).sum(1)
    wabs = torch.zeros(B, dtype=torch.float64).index_add_(0, owner, w * dv.abs())[owner]
    G = rtol * w * (dv.abs() + wabs) + 2.0 ** -126 * (1.0 + dv.abs() + wabs)        # rtol x |terms| + the fp32 flush floor
    if mode == ATT_COS:
        return {"d_pc": torch.zeros_like(pcd).index_add_(0, owner, G[:, None] * prd[col].abs()),
                "d_pr": torch.zeros_like(prd).index_add_(0, col, G[:, None] * pcd[owner].abs())}
    h = pcd[owner] + prd[col]
    assert bool((h != 0).all())                                   # no relu kink: the derivative is defined everywhere
    act = (h > 0).double() * w1.double().abs()
    return {"d_pc": torch.zeros_like(pcd).index_add_(0, owner, G[:, None] * act),
            "d_pr": torch.zeros_like(prd).index_add_(0, col, G[:, None] * act),
            "d_w1": (G[:, None] * torch.relu(h)).sum(0)}


# ------------------------------------------------------------------------------------------------ mirrors of the dispatch
def _lanes(width):
    lp = 8
    while lp < width // 4:
        lp <<= 1
    return lp


def per_pair_form(A, ldpc, ldpr, Fdim, ldfeat, ldout, mode=ATT_MLP):
    """((kind, LPA), (kind, LPF)) of attn_kernel's phase 1 and phase 3: ("vec", lanes per entry), ("gen", 0) for the generic
    phase 1, ("lin", 0) for the linear mode's, ("gen", passes of 64 features) for the generic phase 3."""
    if mode == ATT_LINEAR:
        p1 = ("lin", 0)
    elif A % 4 == 0 and ldpr % 4 == 0 and ldpc % 4 == 0 and A <= 256:
        p1 = ("vec", _lanes(A))
    else:
        p1 = ("gen", 0)
    if Fdim % 4 == 0 and ldfeat % 4 == 0 and ldout % 4 == 0 and Fdim <= 256:
        p3 = ("vec", _lanes(Fdim))
    else:
        p3 = ("gen", (Fdim + 63) // 64)
    return p1, p3


def backward_form(A, Fdim):
    """(LPA, LPF) of attn_backward_kernel (A, Fdim multiples of 4, <= 256)."""
    return _lanes(A), _lanes(Fdim)


def backward_supported(mode, A, Fdim):
    return mode in (ATT_MLP, ATT_COS, ATT_MLP_SCALED) and A % 4 == 0 and Fdim % 4 == 0 and 0 < A <= 256 and 0 < Fdim <= 256


def per_pair_grid(B):
    return (B + 3) // 4


def xcd_remap(blk, nblk):
    """attn_kernel's logical block of hardware block ``blk`` in a grid of ``nblk``."""
    q8, r8, xcd = nblk // 8, nblk % 8, blk % 8
    return (xcd * (q8 + 1) if xcd < r8 else r8 * (q8 + 1) + (xcd - r8) * q8) + blk // 8


LDS_MAX = 160 * 1024


def grouped_form(mode, A, Fdim, ldfeat, ppw, forced="auto"):
    """Mirror of plan_attn_grouped (csrc/attn.hip): (("sc", MODE, CPB, NW) | ("lds", MODE, FO, NPF), LDS bytes), or None where the
    call is refused.  ``forced``: the attn_grouped_kernel option ("auto", "lds", "scalar")."""
    if mode not in (ATT_MLP, ATT_COS, ATT_MLP_SCALED) or A % 4 or A > 256 or Fdim > 256 or not 1 <= ppw <= 32:
        return None
    fvec = Fdim % 4 == 0 and ldfeat % 4 == 0
    pp = 16 if ppw <= 16 else 32
    jobs = (pp // 16) * ((Fdim + 15) // 16)
    lds2 = (64 * (A + Fdim) + pp * 66 + pp + 2 * pp) * 4
    if fvec and lds2 <= LDS_MAX and jobs <= pp and forced != "lds":
        A4 = A // 4
        cpb = 32 if A4 % 32 == 0 else 16 if A4 % 16 == 0 else 8 if A4 % 8 == 0 else 1
        return ("sc", {ATT_MLP: 0, ATT_COS: 2, ATT_MLP_SCALED: 3}[mode], cpb, pp // 4), lds2
    if forced == "scalar":
        return None
    lds = (64 * (A + 4) + 64 * Fdim + ppw * A + A + 64 + 64) * 4
    if lds > LDS_MAX:
        return None
    pieces = (64 * (A // 4 + (Fdim // 4 if fvec else 0)) + 511) // 512
    return ("lds", 2 if mode == ATT_COS else 0, 1 if Fdim <= 64 else 2 if Fdim <= 128 else 4, 4 if pieces <= 4 else 8 if pieces <= 8 else 16), lds


def grouped_grid(B, R, ppw):
    return (B + ppw - 1) // ppw + min(R, B)


def sc_pid_zeroing_waves(A, Fdim, ppw):
    """Waves whose share of attn_grouped_sc_kernel's LDS zeroing loop covers a word of pid[] (thread t zeroes the 16-byte pieces
    t, t + blockDim, ...).  pid[] itself is stored by threads < PP, all in wave 0."""
    pp = 16 if ppw <= 16 else 32
    nthreads = 64 * (pp // 4)
    pid_byte = (64 * (A + Fdim) + pp * 66 + pp) * 4
    assert pid_byte % 8 == 0 and (pid_byte + 8 * pp) % 16 == 0
    return sorted({((pid_byte + 8 * k) // 16 % nthreads) // 64 for k in range(pp)})


def sc_dma_paths(A, Fdim):
    """("readlane" | "divide", swizzled) of the pr tile's DMA and "readlane" | "divide" of the feat tile's."""
    path = lambda x4: "readlane" if x4 in (16, 32, 64) else "divide"
    return (path(A // 4), (A // 4) % 16 == 0), path(Fdim // 4)


# ------------------------------------------------------------------------------------------------ inputs
def wide(x, ld, fill=POISON):
    """``x`` (rows, w) as the first w columns of a (rows, ld) buffer filled with ``fill``."""
    buf = torch.full((x.shape[0], ld), fill, dtype=torch.float32)
    buf[:, :x.shape[1]] = x
    return buf


def expand_csr(rowptr, col, val, pair_row):
    """The per-pair CSR of a shared one: pair b's row is row pair_row[b].  Returns (rowptr, col, val, entry -> shared entry)."""
    rp = rowptr.tolist()
    idx = [torch.arange(rp[r], rp[r + 1]) for r in pair_row.tolist()]
    src = torch.cat(idx) if idx else torch.zeros(0, dtype=torch.long)
    lens = torch.tensor([len(i) for i in idx], dtype=torch.int64)
    xp = torch.zeros(len(idx) + 1, dtype=torch.int64)
    xp[1:] = torch.cumsum(lens, 0)
    return xp, col[src].contiguous(), val[src].contiguous(), src


def make_inputs(mode, A, Fdim, lengths, pairs_per_row, seed, lds=None, bias=True, masked_row_pairs=1, mask_entries=True, I=N_ITEMS):
    """One batch on the CPU.  Row r of the shared CSR has ``lengths[r]`` entries and ``pairs_per_row[r]`` pairs (in shuffled pair
    order); one more row of 9 entries, all out of range, with ``masked_row_pairs`` pairs follows (0: no such row); ``mask_entries=False`` leaves the other rows without an out-of-range column.  ``lds``: dict of leading
    dimensions (pc, pr, feat, out, dout, d_pc, d_pr, d_feat; default width + 4).  Returns a dict: operands (``pc`` .. as (rows, width)
    views of poisoned (rows, ld) buffers ``pc_buf`` ..), the shared CSR, ``pair_row``, the expanded CSR (``x_rowptr`` ..), the float64
    reference (``out64``, ``w64``, ``s64``) and ``w1_shift`` (how many times w1 / pc was halved to bring the spread under 8)."""
    rng = np.random.default_rng(seed)
    lengths, ppr = list(lengths), list(pairs_per_row)
    assert len(lengths) == len(ppr)
    all_masked_row = None
    if masked_row_pairs:
        all_masked_row = len(lengths)
        lengths.append(9)
        ppr.append(masked_row_pairs)
    R = len(lengths)
    rowptr = np.zeros(R + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(lengths)
    hot = np.array([3, 17, 150, I - 1])                              # items rated by most rows: the backward's atomics collide
    cols = []
    for r, n in enumerate(lengths):
        c = rng.permutation(I)[:n]
        if n >= 8:
            rest = c[~np.isin(c, hot)][:n - len(hot)]
            c = rng.permutation(np.concatenate([hot, rest]))
        c = c.astype(np.int64)
        if r == all_masked_row:
            c = np.array([-1, I, I + 7, -5, I + 1, -2, I, -1, 2 * I])
        elif n >= 3 and mask_entries:
            bad = rng.random(n) < 0.08
            bad[int(rng.integers(0, n))] = n >= 7                    # at least one masked entry in every row of 7 or more
            c[bad] = rng.choice([-1, -5, I, I + 7], int(bad.sum()))
        cols.append(c)
    col = np.concatenate(cols).astype(np.int32) if cols else np.zeros(0, np.int32)
    nnz = len(col)
    val = (rng.integers(1, 11, nnz) * 0.5 - 2.9).astype(np.float32)  # -2.4 .. 2.1, never 0
    pair_row = np.repeat(np.arange(R), ppr)
    rng.shuffle(pair_row)
    B = len(pair_row)
    shift, b1 = 0, 0.0
    if mode in (ATT_MLP, ATT_MLP_SCALED):
        pc = (2 * rng.integers(-8, 8, (B, A)) + 1) / 32.0            # odd multiples of 1/32: pc + pr is never 0
        pr = rng.integers(-16, 17, (I, A)) / 16.0
        w1 = rng.integers(-1, 2, A) / 16.0
        b1 = B1
    elif mode == ATT_LINEAR:
        assert A == 1
        pc = (2 * rng.integers(-8, 8, (B, 1)) + 1) / 32.0
        pr = rng.integers(-48, 49, (I, 1)) / 16.0
        w1 = None
    else:                                                           # COS: rows of small dyadic values (multiples of 1/8)
        pc = rng.integers(-8, 9, (B, A)) / 8.0
        pr = rng.integers(-8, 9, (I, A)) / 8.0
        w1 = None
    t = lambda x, dt=torch.float32: None if x is None else torch.tensor(np.asarray(x), dtype=dt)
    rp_t, col_t, val_t, prow_t = torch.from_numpy(rowptr), torch.from_numpy(col), torch.from_numpy(val), torch.from_numpy(pair_row.astype(np.int64))
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn(I, Fdim, generator=g)
    bias_t = torch.randn(Fdim, generator=g) if bias else None
    xp, xcol, xval, xsrc = expand_csr(rp_t, col_t, val_t, prow_t)
    xlens = xp[1:] - xp[:-1]
    while True:                                                     # every entry visible: scale by exact powers of two until it holds
        pcs, w1s = pc, w1
        if mode in (ATT_MLP, ATT_MLP_SCALED):
            w1s = w1 * 2.0 ** -shift
        elif mode == ATT_COS:
            pcs = pc * 2.0 ** -shift
        out64, w64, s64 = attention64(ATT_MLP if mode == ATT_MLP_SCALED else mode, t(pcs, torch.float64), t(pr, torch.float64),
                                      t(w1s, torch.float64), b1, rp_t, col_t, val_t, prow_t, feat.double(),
                                      torch.zeros(Fdim, dtype=torch.float64) if bias_t is None else bias_t.double(), normalize=False)
        spread = 0.0
        for b in range(B):
            x = s64[int(xp[b]):int(xp[b + 1])]
            x = x[torch.isfinite(x)]
            if x.numel():
                spread = max(spread, float(x.max() - x.min()))
        if spread <= SPREAD_MAX or mode == ATT_LINEAR:
            break
        shift += 1
    assert spread <= SPREAD_MAX, (mode, A, spread)
    fin = torch.isfinite(s64)
    assert torch.equal(s64[fin], s64[fin].float().double())         # every logit is exact in fp32: the kernels see the same values
    pc, w1 = pcs, w1s
    if mode == ATT_MLP_SCALED:
        pc, pr, w1 = pc * 2.0 ** -SCALE_LOG2, pr * 2.0 ** -SCALE_LOG2, w1 * 2.0 ** SCALE_LOG2
    ld = {"pc": A + 4, "pr": A + 4, "feat": Fdim + 4, "out": Fdim + 4, "dout": Fdim + 4, "d_pc": A + 4, "d_pr": A + 4, "d_feat": Fdim + 4}
    ld.update(lds or {})
    case = dict(mode=mode, A=A, Fdim=Fdim, I=I, B=B, R=R, b1=b1, ld=ld, w1_shift=shift, spread=spread, all_masked_row=all_masked_row,
                pc_buf=wide(t(pc), ld["pc"]), pr_buf=wide(t(pr), ld["pr"]), feat_buf=wide(feat, ld["feat"]),
                w1_buf=None if w1 is None else wide(t(w1)[None], A + 8)[0], bias_buf=None if bias_t is None else wide(bias_t[None], Fdim + 8)[0],
                rowptr=rp_t, col=col_t, val=val_t, pair_row=prow_t, x_rowptr=xp, x_col=xcol, x_val=xval, x_src=xsrc,
                x_owner=torch.repeat_interleave(torch.arange(B), xlens), out64=out64, w64=w64, s64=s64)
    case["pc"], case["pr"], case["feat"] = case["pc_buf"][:, :A], case["pr_buf"][:, :A], case["feat_buf"][:, :Fdim]
    case["w1"] = None if w1 is None else case["w1_buf"][:A]         # w1 and the bias are the heads of poisoned vectors too
    case["bias"] = None if bias_t is None else case["bias_buf"][:Fdim]
    case["x_ok"] = (xcol >= 0) & (xcol < I)
    rowok = torch.zeros(B, dtype=torch.int64).index_add_(0, case["x_owner"], case["x_ok"].long())
    case["pair_dead"] = rowok == 0                                  # pairs whose row is empty or fully masked: out = bias
    case["pair_empty"] = xlens == 0
    return case


def check_inputs(case):
    """The builder's conditions, asserted on a finished case (test_attn_forms_cpu.py runs this on every table row)."""
    A, Fdim, ld = case["A"], case["Fdim"], case["ld"]
    fin = torch.isfinite(case["s64"])
    assert torch.equal(case["s64"][fin], case["s64"][fin].float().double())
    assert case["spread"] <= SPREAD_MAX
    for name, w in (("pc", A), ("pr", A), ("feat", Fdim)):
        buf = case[name + "_buf"]
        assert buf.shape[1] == ld[name] > w and bool((buf[:, w:] == POISON).all()) and bool((buf[:, :w].abs() < POISON).all()), name
    for name, w in (("w1", A), ("bias", Fdim)):
        if case[name] is not None:
            assert case[name + "_buf"].numel() == w + 8 and bool((case[name + "_buf"][w:] == POISON).all()), name
    assert bool((~case["x_ok"]).any()) == bool((case["s64"] == -float("inf")).any())
    assert torch.equal(case["s64"] == -float("inf"), ~case["x_ok"])
    assert bool((case["val"] != 0).all())


# ------------------------------------------------------------------------------------------------ the checks the GPU tests apply
def fresh_outputs(case, weights=True, nnz=None):
    """(out buffer (B, ldout), weights buffer (nnz + WTS_PAD) or None), every word the sentinel."""
    nnz = case["x_col"].numel() if nnz is None else nnz
    return (torch.full((case["B"], case["ld"]["out"]), SENTINEL, dtype=torch.float32),
            torch.full((nnz + WTS_PAD,), SENTINEL, dtype=torch.float32) if weights else None)


def check_forward(case, out_buf, wts_buf, close, what):
    """``out_buf`` (B, ldout) and ``wts_buf`` (expanded nnz + WTS_PAD words, or None) as a forward kernel left them, on the CPU.
    ``close(got, ref64, tag)`` is the project's bar (test_gpu_basic.assert_close with its defaults)."""
    Fdim, B = case["Fdim"], case["B"]
    out = out_buf[:, :Fdim]
    assert bool((out_buf[:, Fdim:] == SENTINEL).all()), f"{what}: a padding column of out was written"
    unwritten = (out == SENTINEL).any(1)
    assert not bool(unwritten.any()), f"{what}: output rows never written: {unwritten.nonzero().view(-1).tolist()[:8]}"
    dead = case["pair_dead"]
    want = torch.zeros(Fdim) if case["bias"] is None else case["bias"]
    assert torch.equal(out[dead], want.expand(int(dead.sum()), Fdim)), f"{what}: an empty or fully masked row must give the bias bits"
    if wts_buf is not None:
        nnz = case["x_col"].numel()
        assert bool((wts_buf[nnz:] == SENTINEL).all()), f"{what}: weights written past nnz"
        w = wts_buf[:nnz]
        assert bool((w[~case["x_ok"]] == 0.0).all()), f"{what}: a masked entry has a non-zero weight"
        close(w, case["w64"], what + " wts")
    close(out, case["out64"], what + " out")


def backward_reference(case, dout):
    """float64 autograd of attention64 (COS: the dot of the given rows): dict d_pc, d_pr, d_feat, d_w1 (MLP modes), plus the bars."""
    mode = case["mode"]
    pc, pr, feat = (case[k].double().clone().requires_grad_(True) for k in ("pc", "pr", "feat"))
    w1 = case["w1"].double().clone().requires_grad_(True) if case["w1"] is not None else None
    bias = torch.zeros(case["Fdim"], dtype=torch.float64) if case["bias"] is None else case["bias"].double()
    out, w, _ = attention64(ATT_MLP if mode == ATT_MLP_SCALED else mode, pc, pr, w1, case["b1"], case["rowptr"], case["col"], case["val"],
                            case["pair_row"], feat, bias, normalize=False)
    leaves = [pc, pr, feat] + ([w1] if w1 is not None else [])
    grads = torch.autograd.grad((out * dout.double()).sum(), leaves)
    ref = {"d_pc": grads[0], "d_pr": grads[1], "d_feat": grads[2]}
    if w1 is not None:
        ref["d_w1"] = grads[3]
    ok = case["x_ok"]
    bars = backward_bars(mode, case["pc"], case["pr"], case["w1"], case["x_col"].long()[ok], case["x_owner"][ok], case["x_val"][ok],
                         case["feat"], dout, w.detach()[ok])
    return ref, bars


def fresh_gradients(case):
    ld, B, I, A = case["ld"], case["B"], case["I"], case["A"]
    z = lambda rows, l, w: wide(torch.zeros(rows, w), l, SENTINEL)           # accumulated into: zeros inside, sentinel padding
    return dict(d_pc=torch.full((B, ld["d_pc"]), SENTINEL), d_pr=z(I, ld["d_pr"], A), d_feat=z(I, ld["d_feat"], case["Fdim"]),
                d_w1_part=torch.full((B, A), SENTINEL))


def check_backward(case, dout, got, close, bar_check, what):
    """``got``: the gradient buffers of fresh_gradients() after the kernel.  ``bar_check(got, ref, bar, tag)`` applies an
    elementwise bar; ``close`` the default one."""
    A, Fdim = case["A"], case["Fdim"]
    ref, bars = backward_reference(case, dout)
    for name, w in (("d_pc", A), ("d_pr", A), ("d_feat", Fdim)):
        assert bool((got[name][:, w:] == SENTINEL).all()), f"{what}: padding of {name} written"
    d_pc = got["d_pc"][:, :A]
    assert not bool((d_pc == SENTINEL).any()), f"{what}: d_pc rows never written"
    assert bool((d_pc[case["pair_dead"]] == 0).all()), f"{what}: a pair without a valid entry must get a zero d_pc row"
    close(got["d_feat"][:, :Fdim], ref["d_feat"], what + " d_feat")
    bar_check(d_pc, ref["d_pc"], bars["d_pc"], what + " d_pc")
    bar_check(got["d_pr"][:, :A], ref["d_pr"], bars["d_pr"], what + " d_pr")
    if "d_w1" in ref:
        part = got["d_w1_part"]
        assert not bool((part == SENTINEL).any()), f"{what}: d_w1_part rows never written"
        assert bool((part[case["pair_dead"]] == 0).all())
        bar_check(part.double().sum(0), ref["d_w1"], bars["d_w1"], what + " d_w1")


# ------------------------------------------------------------------------------------------------ case tables
def _ld(**kw):
    return tuple(sorted(kw.items()))


PPCase = collections.namedtuple("PPCase", "mode A Fdim B lds bias seed")         # lds: leading dimensions, _ld(pc=.., pr=.., ..)
BWCase = collections.namedtuple("BWCase", "mode A Fdim B lds seed")
GCase = collections.namedtuple("GCase", "mode A Fdim ldfeat ppw force seed")

A_VEC, A_GEN = (4, 20, 32, 36, 64, 68, 100, 128, 132, 192, 256), (1, 3, 10, 30, 260)
F_VEC, F_GEN = (4, 20, 32, 36, 64, 68, 100, 128, 132, 256), (1, 3, 50, 70, 130, 260)
PP_BATCHES = (1, 3, 4, 5, 28, 29, 33, 61, 67)                     # grids of 1, 1, 1, 2, 7, 8, 9, 16, 17 blocks


def _per_pair_cases():
    rng = np.random.default_rng(2024)
    modes = (ATT_MLP, ATT_MLP_SCALED, ATT_COS)
    fdims = list(rng.permutation(F_VEC + F_GEN)) * 2
    cases, n = [], 0
    for k, A in enumerate(A_VEC + A_GEN):
        if A == 1:
            continue
        for rep in range(2):                                        # every A twice: a large batch (all row lengths) and a small grid
            Fdim = int(fdims[n % len(fdims)])
            B = PP_BATCHES[4 + k % 5] if rep == 0 else PP_BATCHES[k % 4]
            pad = 4 if n % 3 else 8
            lds = _ld(pc=A + pad, pr=A + 4, feat=Fdim + pad, out=Fdim + 4)
            cases.append(PPCase(modes[n % 3], A, Fdim, B, lds, n % 4 != 1, 100 + n))
            n += 1
    for k, Fdim in enumerate(F_VEC + F_GEN):                        # every Fdim at least once on a full batch
        if not any(c.Fdim == Fdim and c.B >= 28 for c in cases):
            A = A_VEC[(3 * k) % len(A_VEC)]
            cases.append(PPCase(modes[k % 3], A, Fdim, PP_BATCHES[4 + k % 5], _ld(pc=A + 4, pr=A + 8, feat=Fdim + 8, out=Fdim + 4), k % 2 == 0, 300 + k))
    # A = 1: the linear mode, and the generic MLP / COS phase 1
    for k, (mode, Fdim, B) in enumerate([(ATT_LINEAR, 64, 33), (ATT_LINEAR, 50, 5), (ATT_LINEAR, 132, 61), (ATT_MLP, 36, 29), (ATT_COS, 3, 4)]):
        cases.append(PPCase(mode, 1, Fdim, B, _ld(pc=5 if k % 2 else 1 + 4, pr=2, feat=Fdim + 4, out=Fdim + 4), k != 1, 400 + k))
    # a leading dimension that is not a multiple of 4 sends a vector shape down the generic path
    cases.append(PPCase(ATT_MLP, 64, 64, 29, _ld(pc=68, pr=65, feat=68, out=68), True, 500))
    cases.append(PPCase(ATT_COS, 64, 64, 33, _ld(pc=66, pr=68, feat=68, out=68), True, 501))
    cases.append(PPCase(ATT_MLP_SCALED, 128, 64, 28, _ld(pc=132, pr=132, feat=65, out=68), False, 502))
    cases.append(PPCase(ATT_MLP, 32, 128, 67, _ld(pc=36, pr=36, feat=132, out=131), True, 503))
    return cases


def _backward_cases():
    reps = {8: (4, 20, 32), 16: (36, 64), 32: (100, 128), 64: (132, 256)}
    modes = (ATT_MLP, ATT_MLP_SCALED, ATT_COS)
    cases, n = [], 0
    for lpa in (8, 16, 32, 64):
        for lpf in (8, 16, 32, 64):
            A, Fdim = reps[lpa][n % len(reps[lpa])], reps[lpf][(n // 2 + lpa // 8) % len(reps[lpf])]
            lds = _ld(pc=A + 4, pr=A + 8, feat=Fdim + 4, dout=Fdim + 8, d_pc=A + 4, d_pr=A + 1 + n % 3, d_feat=Fdim + 3 - n % 3)
            cases.append(BWCase(modes[n % 3], A, Fdim, 29 if n % 2 == 0 else 9, lds, 700 + n))
            n += 1
    for k, (A, Fdim) in enumerate([(20, 36), (100, 132), (4, 4), (32, 20), (256, 100), (128, 4)]):   # idle lanes on both sides; the rest of the sizes
        cases.append(BWCase(modes[k % 3], A, Fdim, 29, _ld(pc=A + 4, pr=A + 4, feat=Fdim + 8, dout=Fdim + 4, d_pc=A + 8, d_pr=A + 2, d_feat=Fdim + 1), 750 + k))
    return cases


def _grouped_cases():
    sc_A = {32: (128, 256), 16: (64, 192), 8: (32, 96), 1: (4, 20, 100)}
    sc_F = (4, 20, 64, 68, 100, 132, 256)
    cases, n = [], 0
    for mode in (ATT_MLP, ATT_COS, ATT_MLP_SCALED):                 # the 24 scalar-operand instantiations
        for cpb in (32, 16, 8, 1):
            for k, ppw in enumerate((16, 32) if n % 2 else (5, 17)):
                A = sc_A[cpb][(n + k) % len(sc_A[cpb])]
                Fdim = sc_F[(n + 3 * k) % len(sc_F)]
                cases.append(GCase(mode, A, Fdim, Fdim + 4, ppw, "scalar", 800 + 2 * n + k))
            n += 1
    # the swizzled divide path (A = 192), the readlane paths on both tiles, one pair per workgroup, > 64 KiB of LDS, and shapes whose
    # pid[] words are zeroed by another wave than the one that stores them
    for k, (mode, A, Fdim, ppw) in enumerate([(ATT_MLP, 192, 64, 16), (ATT_COS, 192, 132, 32), (ATT_MLP_SCALED, 64, 256, 1), (ATT_MLP, 128, 128, 17),
                                               (ATT_MLP_SCALED, 256, 256, 32), (ATT_COS, 256, 64, 5), (ATT_MLP, 8, 20, 16), (ATT_MLP_SCALED, 20, 64, 5),
                                               (ATT_COS, 128, 68, 32), (ATT_MLP, 100, 100, 1), (ATT_MLP_SCALED, 96, 4, 32), (ATT_COS, 32, 20, 16)]):
        cases.append(GCase(mode, A, Fdim, Fdim + 8, ppw, "scalar", 900 + k))
    # the 18 LDS-broadcast instantiations: FO by Fdim, NPF by A + (Fdim when it is staged as 16-byte pieces)
    lds_shapes = {(1, 4): (32, 20), (1, 8): (128, 64), (1, 16): (256, 20), (2, 4): (20, 100), (2, 8): (128, 100), (2, 16): (192, 100),
                  (4, 4): (64, 130), (4, 8): (32, 200), (4, 16): (100, 256)}
    ppws = (1, 5, 16, 17, 32)
    for mode in (ATT_MLP, ATT_COS):
        for (fo, npf), (A, Fdim) in lds_shapes.items():
            cases.append(GCase(mode, A, Fdim, Fdim + 4, ppws[n % 5], "lds", 1000 + n))
            n += 1
    for k, (mode, A, Fdim, ldfeat, ppw) in enumerate([(ATT_MLP_SCALED, 128, 64, 68, 32), (ATT_MLP, 64, 50, 54, 16), (ATT_COS, 96, 130, 131, 17),
                                                       (ATT_MLP, 4, 64, 65, 5), (ATT_COS, 192, 256, 260, 5), (ATT_MLP, 256, 200, 204, 1)]):
        cases.append(GCase(mode, A, Fdim, ldfeat, ppw, "lds", 1100 + k))
    # option at "auto": Fdim % 4 != 0 (or ldfeat % 4 != 0) falls to the LDS form, the rest takes the scalar-operand form
    for k, (mode, A, Fdim, ldfeat, ppw) in enumerate([(ATT_MLP, 64, 50, 52, 16), (ATT_COS, 32, 130, 132, 5), (ATT_MLP_SCALED, 128, 64, 67, 32),
                                                       (ATT_MLP_SCALED, 128, 64, 68, 17)]):
        cases.append(GCase(mode, A, Fdim, ldfeat, ppw, "auto", 1200 + k))
    return cases


PER_PAIR_CASES, BACKWARD_CASES, GROUPED_CASES = _per_pair_cases(), _backward_cases(), _grouped_cases()


def case_id(c):
    d = c._asdict()
    s = f"{MODE_NAMES[d['mode']]}-A{d['A']}-F{d['Fdim']}"
    if "B" in d:
        s += f"-B{d['B']}"
    if "ppw" in d:
        s += f"-ppw{d['ppw']}-{d['force']}-ld{d['ldfeat']}"
    if "lds" in d:
        s += "-" + "".join(f"{k}{v}" for k, v in d["lds"] if k in ("pc", "pr", "feat", "out"))
    return s + f"-s{d['seed']}"


def _rows_for(n_pairs, seed):
    """Lengths and pairs per row for ``n_pairs`` pairs: every length of LENGTHS when there are that many pairs (the surplus shares
    rows); else one pair per row, the lengths picked from a seed-dependent start so that the small batches cover the list between them."""
    n = len(LENGTHS)
    if n_pairs >= n:
        return list(LENGTHS), [n_pairs // n + (1 if r < n_pairs % n else 0) for r in range(n)]
    return [LENGTHS[(seed * 5 + 7 * k) % n] for k in range(n_pairs)], [1] * n_pairs


@functools.lru_cache(maxsize=None)
def per_pair_inputs(c):
    masked = 1 if c.B >= 4 else 0                                   # one pair on the all-masked row
    lengths, ppr = _rows_for(c.B - masked, c.seed)
    case = make_inputs(c.mode, c.A, c.Fdim, lengths, ppr, c.seed, lds=dict(c.lds), bias=c.bias, masked_row_pairs=masked)
    assert case["B"] == c.B, (case["B"], c.B)
    return case


@functools.lru_cache(maxsize=None)
def backward_inputs(c):
    case = per_pair_inputs(PPCase(c.mode, c.A, c.Fdim, c.B, c.lds, True, c.seed))
    g = torch.Generator().manual_seed(c.seed)
    dout = torch.randn(case["B"], c.Fdim, generator=g)
    return case, dout, wide(dout, dict(c.lds)["dout"])


GROUPED_LENGTHS = LENGTHS + (40,)                                # the last row has entries and no pair: it gets no workgroup


def grouped_pairs_per_row(ppw):
    """Group sizes 1 .. 5, ppw - 1 and ppw, rows of several groups with a partly filled last one, a row without a pair."""
    counts = [1, 2, 3, 4, 5, max(ppw - 1, 1), ppw, 2 * ppw + 1, ppw + 3]
    return [counts[r % len(counts)] for r in range(len(LENGTHS))] + [0]


@functools.lru_cache(maxsize=None)
def grouped_inputs(c):
    return make_inputs(c.mode, c.A, c.Fdim, GROUPED_LENGTHS, grouped_pairs_per_row(c.ppw), c.seed,
                       lds={"feat": c.ldfeat, "out": c.Fdim + (4 if c.seed % 2 else 5)}, masked_row_pairs=3)
