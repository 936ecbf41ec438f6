"""Reference, inputs and emulator for the cross-product attention of csrc/attn_cross.hip (CPU only: nothing here touches a GPU).

The table formulation restated in float64 — the logit table ST (rated x candidate), then per listed user a gather of ST rows, a
column softmax and the rating-weighted sum — next to ``attn_forms_ref.attention64`` on the expanded (user, candidate) pairs, which is
the reference the GPU test holds ``native.attn_cross`` to.  ``make_cross_case`` builds on ``attn_forms_ref.make_inputs`` (its CSR with
every row length, masked entries, an all-masked row, poisoned operand buffers, exact dyadic logits) and adds a candidate catalogue
made by the same recipe.  ``emulate_cross`` walks the kernel's indices in fp32 with one optional seeded defect;
tests/test_attn_cross_cpu.py shows that the right walk passes ``check_forward`` and that each defect fails it."""
import functools

import numpy as np
import torch

import attn_forms_ref as R

DEFECTS = ("table_not_transposed", "last_candidate_tile_dropped", "col_not_masked", "val_left_out", "cand_ids_ignored",
           "block_offset_not_on_user_rows")
CAND_TILE = 128           # candidates per workgroup of attn_cross_kernel


def table64(mode, pc, pr, w1, b1):
    """ST (I_r, I_c) float64: ST[e, i] = the logit of candidate i against rated item e (rows given as the kernels get them)."""
    return R.scores64(R.ATT_MLP if mode == R.ATT_MLP_SCALED else mode, pc.double(), pr.double(), None if w1 is None else w1.double(), b1,
                      normalize=False).t().contiguous()


def cross64(ST, rowptr, col, val, user_rows, cand_ids, feat, bias):
    """out (U * I, Fdim) float64 from the table: row u * I + j = bias + sum_e softmax_e(ST[col_e, cand_j]) val_e feat[col_e]; masked
    entries (col outside the table's rows) dropped; a user without a valid entry gets the bias."""
    Ir, Ic = ST.shape
    cands = torch.arange(Ic) if cand_ids is None else cand_ids.long()
    rp = rowptr.tolist()
    out = []
    for r in user_rows.tolist():
        c, v = col[rp[r]:rp[r + 1]].long(), val[rp[r]:rp[r + 1]].double()
        ok = (c >= 0) & (c < Ir)
        if not bool(ok.any()):
            out.append(bias.double().expand(cands.numel(), -1))
            continue
        S = ST[c[ok]][:, cands]                                        # (entries, I): coalesced rows of the table
        W = torch.softmax(S, 0)
        out.append((W * v[ok][:, None]).t() @ feat.double()[c[ok]] + bias.double())
    return torch.cat(out) if out else torch.zeros((0, feat.shape[1]), dtype=torch.float64)


def _candidates(mode, A, Ic, shift, rng):
    """The candidate catalogue's projected rows, by make_inputs' recipe for ``pc`` (and its power-of-two scale for the cosine rows)."""
    if mode in (R.ATT_MLP, R.ATT_MLP_SCALED):
        pc = (2 * rng.integers(-8, 8, (Ic, A)) + 1) / 32.0
        if mode == R.ATT_MLP_SCALED:
            pc = pc * 2.0 ** -R.SCALE_LOG2
    elif mode == R.ATT_LINEAR:
        pc = (2 * rng.integers(-8, 8, (Ic, 1)) + 1) / 32.0
    else:
        pc = rng.integers(-8, 9, (Ic, A)) / 8.0 * 2.0 ** -shift
    return torch.tensor(pc, dtype=torch.float32)


def make_cross_case(mode, A, Fdim, Ic, seed, lengths=R.LENGTHS, cand_subset=False, bias=True, Ir=R.N_ITEMS, ldfeat=None):
    """One cross-product batch on the CPU.  The users' CSR is make_inputs' (one row per length, then the all-masked row; entries of
    rows >= 3 partly out of range); ``user_rows`` lists every row once in shuffled order plus a repeated and an out-of-order user;
    ``cand_subset``: ``cand_ids`` = a shuffled subset of the catalogue with one repeat (else None: candidates 0 .. I_c - 1);
    ``ldfeat``: the feat buffer's leading dimension (default Fdim + 4; no multiple of 4 takes the kernel's scalar staging).  The dict
    has what attn_forms_ref.check_forward reads (B = U * I pairs, ``out64`` = attention64 on the expanded pairs, ``pair_dead``, ...),
    the table ``st64`` and the kernel's operands."""
    base = R.make_inputs(mode, A, Fdim, lengths, [1] * len(lengths), seed, bias=bias, masked_row_pairs=1, I=Ir,
                         lds=None if ldfeat is None else {"feat": ldfeat})
    rng = np.random.default_rng(seed + 7919)
    pc = _candidates(mode, A, Ic, base["w1_shift"], rng)
    nrows = base["R"]
    order = rng.permutation(nrows).tolist()
    user_rows = torch.tensor(order + [order[0], order[len(order) // 2], 0], dtype=torch.int64)     # repeats, any order
    cand_ids = None
    if cand_subset:
        keep = rng.permutation(Ic)[:max(1, (2 * Ic) // 3)]
        cand_ids = torch.tensor(np.concatenate([keep, keep[:1]]), dtype=torch.int64)                # a shuffled subset with a repeat
    cands = torch.arange(Ic) if cand_ids is None else cand_ids
    U, I = user_rows.numel(), cands.numel()
    st64 = table64(mode, pc, base["pr"], base["w1"], base["b1"])
    assert torch.equal(st64, st64.float().double())                    # every logit is exact in fp32
    bias64 = torch.zeros(Fdim, dtype=torch.float64) if base["bias"] is None else base["bias"].double()
    # the reference: attention64 on the expanded pairs (pair u * I + j = candidate cand_j against the set of user_rows[u])
    pair_row = user_rows.repeat_interleave(I)
    out64, _, _ = R.attention64(R.ATT_MLP if mode == R.ATT_MLP_SCALED else mode, pc.double()[cands.repeat(U)], base["pr"].double(),
                                None if base["w1"] is None else base["w1"].double(), base["b1"], base["rowptr"], base["col"], base["val"],
                                pair_row, base["feat"].double(), bias64, normalize=False)
    rp = base["rowptr"]
    okc = (base["col"] >= 0) & (base["col"] < Ir)
    row_valid = torch.tensor([bool(okc[int(rp[r]):int(rp[r + 1])].any()) for r in range(nrows)])
    case = dict(mode=mode, A=A, Fdim=Fdim, Ic=Ic, Ir=Ir, I=I, U=U, B=U * I, n_rows=nrows, b1=base["b1"], bias=base["bias"], bias_buf=base["bias_buf"],
                pc=pc, pc_buf=R.wide(pc, pc.shape[1] + 4), pr=base["pr"], pr_buf=base["pr_buf"], w1=base["w1"], w1_buf=base["w1_buf"],
                feat=base["feat"], feat_buf=base["feat_buf"], rowptr=base["rowptr"], col=base["col"], val=base["val"],
                user_rows=user_rows, cand_ids=cand_ids, st64=st64, out64=out64, pair_dead=~row_valid[pair_row],
                ld={"pc": pc.shape[1] + 4, "pr": base["ld"]["pr"], "feat": base["ld"]["feat"], "out": Fdim + 4, "st": Ic + 4},
                x_col=torch.zeros(0, dtype=torch.int32), all_masked_row=base["all_masked_row"])
    return case


@functools.lru_cache(maxsize=None)
def cross_inputs(mode, A, Fdim, Ic, seed, cand_subset, ldfeat=None, bias=True):
    return make_cross_case(mode, A, Fdim, Ic, seed, cand_subset=cand_subset, ldfeat=ldfeat, bias=bias)


def fresh_out(case):
    """The (U * I, ldout) output buffer before the call: every word the sentinel."""
    return R.fresh_outputs(case, weights=False, nnz=0)[0]


def emulate_cross(case, st, defect=None, users_per_call=None):
    """attn_cross_kernel's index walk in fp32 on the CPU: ``st`` (I_r, I_c) fp32 table, one "call" per block of ``users_per_call``
    listed users (the model's blocking; None = one call), workgroups of CAND_TILE candidates, the exact column maximum first, then
    exp / sum / weighted aggregation.  ``defect``: one of DEFECTS, or None for the right walk.  Returns the output buffer."""
    assert defect is None or defect in DEFECTS
    Fdim, I, U, Ir = case["Fdim"], case["I"], case["U"], case["Ir"]
    buf = fresh_out(case)
    feat, val, col, rp = case["feat"].float(), case["val"].float(), case["col"].long(), case["rowptr"].tolist()
    bias = torch.zeros(Fdim) if case["bias"] is None else case["bias"].float()
    cands = torch.arange(I) if (case["cand_ids"] is None or defect == "cand_ids_ignored") else case["cand_ids"].long()
    step = U if users_per_call is None else users_per_call
    ntiles = (I + CAND_TILE - 1) // CAND_TILE
    if defect == "last_candidate_tile_dropped" and I % CAND_TILE:
        ntiles -= 1
    for u0 in range(0, U, step):
        rows = case["user_rows"][u0:u0 + step]
        if defect == "block_offset_not_on_user_rows":
            rows = case["user_rows"][0:rows.numel()]                   # the block's users read from the head of the list
        for k, r in enumerate(rows.tolist()):
            c, v = col[rp[r]:rp[r + 1]], val[rp[r]:rp[r + 1]]
            if defect == "col_not_masked":
                ok = torch.ones_like(c, dtype=torch.bool)
                c = c.clamp(0, Ir - 1)
            else:
                ok = (c >= 0) & (c < Ir)
            for tile in range(ntiles):
                j = torch.arange(tile * CAND_TILE, min(I, (tile + 1) * CAND_TILE))
                o = buf[(u0 + k) * I + j]
                if not bool(ok.any()):
                    o[:, :Fdim] = bias
                else:
                    cj = cands[j]
                    S = st[cj][:, c[ok]].t() if defect == "table_not_transposed" else st[c[ok]][:, cj]
                    m = S.max(0).values
                    P = torch.exp(S - m)
                    l = P.sum(0)
                    PV = P if defect == "val_left_out" else P * v[ok][:, None]
                    o[:, :Fdim] = (PV.t() @ feat[c[ok]]) / l[:, None] + bias
                buf[(u0 + k) * I + j] = o
    return buf
